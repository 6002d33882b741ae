"""umicollapse -m fastq with the staging on the device, the CLI's side of it, without a GPU: the CLI runs
against a stub libumihip.so (built here, beside a copy of the binary) that keeps HIP's rule that the
current device is per thread and starts at 0.  The stub's hipMalloc refuses memory on any other device
than the context's, so a CLI that allocated before selecting `--device N` fails.  Also: a length
problem is reported without a GPU, and the earlier of a length and a character problem is named."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")

STUB = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
typedef struct { int device; } umi_ctx;
static __thread int cur_device = 0;   /* HIP: per thread, 0 until hipSetDevice */
static int ctx_device = -1;
static char err[256] = "";
const char *umi_last_error(void) { return err; }
int umi_ctx_create_multi(const int *ids, int n, umi_ctx **out)
{
    umi_ctx *c = (umi_ctx *)malloc(sizeof(umi_ctx));
    c->device = ids[0];
    ctx_device = ids[0];
    *out = c;
    return 0;
}
int umi_ctx_set_option(umi_ctx *c, const char *name, int64_t v) { return 0; }
int umi_stage_reads_wide(void) { return -1; }
int umi_dedup_batch_wide(void) { return -1; }
int umi_dedup_seqs(umi_ctx *c, const uint64_t *k, const uint64_t *nm, int w, const int32_t *f, const uint64_t *off,
                   const int32_t *bl, uint64_t nb, int kk, float p, int a, int32_t adj, uint8_t *kept, uint32_t *root,
                   void *st) { memset(st, 0, 128); return 0; }
int umi_dedup_seqs_device(umi_ctx *c, const uint64_t *k, const uint64_t *nm, int w, const int32_t *f, const uint64_t *off,
                          const int32_t *bl, uint64_t nb, int kk, float p, int a, int32_t adj, uint8_t *kept,
                          uint32_t *root, void *s, void *st) { memset(st, 0, 128); return 0; }
int umi_stage_seqs(umi_ctx *c, const uint8_t *t, const uint64_t *sp, const uint64_t *qp, const uint32_t *len, uint64_t n,
                   int w, int merge, uint64_t *k, uint64_t *nm, int32_t *f, uint64_t *rep, uint32_t *eor, uint64_t *off,
                   int32_t *bl, uint64_t *ne, uint64_t *nb, int *any_n)
{ *ne = 0; *nb = 0; *any_n = 0; off[0] = 0; return 0; }
int umi_stage_seqs_device(umi_ctx *c, const uint8_t *t, const uint64_t *sp, const uint64_t *qp, const uint32_t *len,
                          uint64_t n, int w, int merge, uint64_t *k, uint64_t *nm, int32_t *f, uint64_t *rep,
                          uint32_t *eor, uint64_t *off, int32_t *bl, uint64_t *ne, uint64_t *nb, int *any_n, void *s)
{ *ne = 0; *nb = 0; *any_n = 0; off[0] = 0; return 0; }
int hipSetDevice(int d) { cur_device = d; return 0; }
int hipMalloc(void **p, size_t bytes)
{
    if (cur_device != ctx_device) {
        fprintf(stderr, "stub: hipMalloc on device %d, the context is on device %d\n", cur_device, ctx_device);
        return 1;
    }
    *p = malloc(bytes);
    return *p ? 0 : 2;
}
int hipMemcpy(void *d, const void *s, size_t n, int kind) { memcpy(d, s, n); return 0; }
"""


@pytest.fixture(scope="module")
def stub_cli(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])
    d = tmp_path_factory.mktemp("stubbed")
    (d / "bin").mkdir()
    shutil.copy(CLI, d / "bin" / "umicollapse")
    (d / "stub.c").write_text(STUB)
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", "-o", str(d / "libumihip.so"), str(d / "stub.c")])
    return str(d / "bin" / "umicollapse")


def run(cli, args):
    return subprocess.run([cli] + args, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("device", ["0", "3"])
def test_buffers_on_the_context_device(stub_cli, tmp_path, device):
    src = tmp_path / "a.fq"
    src.write_bytes(b"@a\nACGT\n+\nIIII\n@b\nACGA\n+\nIIII\n")
    r = run(stub_cli, ["-m", "fastq", "-i", str(src), "-o", str(tmp_path / "o.fq"), "--stage", "gpu",
                       "--device", device])
    assert r.returncode == 0, r.stderr
    assert "staging (gpu)" in r.stderr


@pytest.mark.parametrize("text,want", [
    (b"@a\n" + b"A" * 300 + b"\n+\n" + b"I" * 300 + b"\n", "FASTQ record 1: 300 bases, more than 256"),
    (b"@a\nACGT\n+\nIIII\n@b\nAC\n+\nII\n", "FASTQ record 2: 2 bases, shorter than -u 3"),
    (b"@a\nACGT\n+\nIIII\n@b\nAC.T\n+\nIIII\n@c\nA\n+\nI\n", "Unknown character in sequence: 46 (FASTQ record 2)"),
    (b"@a\nACGT\n+\nIIII\n@c\nA\n+\nI\n@b\nAC.T\n+\nIIII\n", "FASTQ record 2: 1 bases, shorter than -u 3"),
])
@pytest.mark.parametrize("stage", ["auto", "gpu", "host"])
def test_length_problems_need_no_gpu(tmp_path, text, want, stage):
    """with no GPU visible at all: the same status and message on every side"""
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])
    src = tmp_path / "bad.fq"
    src.write_bytes(text)
    r = subprocess.run([CLI, "-m", "fastq", "-i", str(src), "-o", str(tmp_path / "o.fq"), "-u", "3", "--stage", stage],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 101, r.stderr
    assert r.stderr.strip().splitlines()[-1] == "umicollapse: " + want
