"""umi_correct_umis / umi_correct_umis_device on the GPU against tests/whitelist_model.py: match, best,
second, out and counts, all by exact equality."""

import numpy as np
import pytest

import whitelist_model as wm

pytestmark = pytest.mark.gpu

TILE = 1024  # CORR_TILE of umihip_internal.h: listed UMIs in LDS at a time
FIELDS = ("match", "best", "second", "out", "counts")


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def same(got, exp, fields=FIELDS):
    for f in fields:
        a, b = np.asarray(got[f]), np.asarray(exp[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        bad = np.flatnonzero(a != b)
        assert not len(bad), (f, bad[:10], a[bad[:10]], b[bad[:10]])


def case(seed, umi_len, n_wl, n):
    rng = np.random.default_rng(seed)
    wl = wm.random_list(rng, n_wl, umi_len)
    return wl, wm.noisy_reads(rng, wl, umi_len, n)


@pytest.mark.parametrize("n_wl", [1, 2, 64, 65, 1500, TILE + 1])
@pytest.mark.parametrize("umi_len", [1, 8, 12, 21, 22, 43, 64, 65, 85])
def test_lengths_and_list_sizes(ctx, umi_len, n_wl):
    wl, reads = case(1000 * umi_len + n_wl, umi_len, n_wl, 3000)
    exp = wm.correct(reads, umi_len, wl, 2, 1)
    same(ctx.correct_umis(reads, umi_len, wl, 2, 1), exp)
    if umi_len >= 8 and n_wl >= 64:  # (the inputs are what they are meant to be: every verdict occurs)
        assert all(int(c) > 0 for c in exp["counts"])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 20000])
def test_read_counts(ctx, n):
    wl, reads = case(77 + n, 12, 96, n)
    got = ctx.correct_umis(reads, 12, wl)
    same(got, wm.correct(reads, 12, wl))
    assert len(got["match"]) == n and int(got["counts"].sum()) == n


@pytest.fixture(scope="module")
def grid_input():
    return case(4242, 12, 200, 3000)


@pytest.mark.parametrize("min_distance", [0, 1, 2, 13])
@pytest.mark.parametrize("max_mismatches", [0, 1, 3, 12])
def test_parameter_grid(ctx, grid_input, max_mismatches, min_distance):
    wl, reads = grid_input
    same(ctx.correct_umis(reads, 12, wl, max_mismatches, min_distance), wm.correct(reads, 12, wl, max_mismatches, min_distance))


def test_beyond_any_distance(ctx, grid_input):
    wl, reads = grid_input
    big = 2 ** 31 - 1
    same(ctx.correct_umis(reads, 12, wl, big, 0), wm.correct(reads, 12, wl, 12, 0))
    got = ctx.correct_umis(reads, 12, wl, 1, big)
    assert (got["match"] == -1).all() and int(got["counts"][2]) == len(reads) // 12


def test_ties_between_two_listed_umis(ctx):
    # the two first entries are one base apart; a read that has a third base there is 1 from both
    wl = ["ACGTACGTACGT", "ACGTACGTACGA", "TTTTTTTTTTTT", "ACGTACGTACGA"]
    reads = ["ACGTACGTACGC", "ACGTACGTACGN", "ACGTACGTACGT", "ACGTACGTACGA", "TTTTTTTTTTTA"] * 40
    raw = np.frombuffer("".join(reads).encode(), np.uint8)
    for md in (0, 1):
        got = ctx.correct_umis(raw, 12, wl, 1, md)
        same(got, wm.correct(raw, 12, wl, 1, md))
    got = ctx.correct_umis(raw, 12, wl, 1, 0)
    assert list(got["match"][:5]) == [0, 0, 0, 1, 2] and list(got["best"][:5]) == [1, 1, 0, 0, 1]
    assert list(got["second"][:5]) == [1, 1, 1, 0, 9]


# ---- the device form ------------------------------------------------------------------------------------

def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def device_call(ctx, reads, umi_len, wl, mm=1, md=1, shift=0, in_place=False, want_out=True, want_best=True,
                want_second=True):
    """the device form on buffers with a guard band filled beforehand; returns the result dict and checks
    that nothing outside the outputs' own extent (and no output that was not asked for) was written"""
    import torch
    n, G, fill = len(reads) // umi_len, 64, 0x5A
    raw = torch.full((len(reads) + shift + G,), fill, dtype=torch.uint8, device="cuda:0")
    raw[shift:shift + len(reads)] = dev(reads)
    out = torch.full((len(reads) + G,), fill, dtype=torch.uint8, device="cuda:0")
    match = torch.full((n + G,), -0x5A5A5A5B, dtype=torch.int32, device="cuda:0")
    best = torch.full((n + G,), fill, dtype=torch.uint8, device="cuda:0")
    second = torch.full((n + G,), fill, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    d_in = raw.data_ptr() + shift
    d_out = d_in if in_place else (out.data_ptr() if want_out else 0)
    counts = ctx.correct_umis_device(d_in, n, umi_len, wl, mm, md, d_out, match.data_ptr(),
                                     best.data_ptr() if want_best else 0, second.data_ptr() if want_second else 0)
    torch.cuda.synchronize()
    raw_h, out_h, match_h, best_h, second_h = (t.cpu().numpy() for t in (raw, out, match, best, second))
    assert (match_h[n:] == -0x5A5A5A5B).all()
    assert (raw_h[:shift] == fill).all() and (raw_h[shift + len(reads):] == fill).all()
    assert (out_h[len(reads) if want_out and not in_place else 0:] == fill).all()
    assert (best_h[n if want_best else 0:] == fill).all()
    assert (second_h[n if want_second else 0:] == fill).all()
    if not in_place:
        assert (raw_h[shift:shift + len(reads)] == reads).all()
    res = {"match": match_h[:n], "counts": counts}
    if in_place:
        res["out"] = raw_h[shift:shift + len(reads)]
    elif want_out:
        res["out"] = out_h[:len(reads)]
    if want_best:
        res["best"] = best_h[:n]
    if want_second:
        res["second"] = second_h[:n]
    return res


@pytest.fixture(scope="module")
def dev_input():
    wl, reads = case(99, 22, 300, 3000)
    return wl, reads, wm.correct(reads, 22, wl, 2, 1)


@pytest.mark.parametrize("kw", [
    dict(),
    dict(in_place=True),
    dict(want_out=False),
    dict(want_best=False),
    dict(want_second=False),
    dict(want_out=False, want_best=False, want_second=False),
    dict(shift=1),
    dict(shift=1, in_place=True),
    dict(shift=3, want_best=False),
], ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()) or "all")
def test_device_form_and_optional_outputs(ctx, dev_input, kw):
    wl, reads, exp = dev_input
    got = device_call(ctx, reads, 22, wl, 2, 1, **kw)
    same(got, exp, [f for f in FIELDS if f in got])


def test_host_form_equals_device_form(ctx, dev_input):
    wl, reads, exp = dev_input
    host = ctx.correct_umis(reads, 22, wl, 2, 1)
    device = device_call(ctx, reads, 22, wl, 2, 1)
    same(host, device)
    same(host, exp)


def test_device_form_on_a_stream(ctx, dev_input):
    import torch
    wl, reads, exp = dev_input
    n = len(reads) // 22
    s = torch.cuda.Stream()
    d_in, d_match = dev(reads), torch.zeros(n, dtype=torch.int32, device="cuda:0")
    s.wait_stream(torch.cuda.default_stream())
    counts = ctx.correct_umis_device(d_in.data_ptr(), n, 22, wl, 2, 1, 0, d_match.data_ptr(), stream=s.cuda_stream)
    # (the call has synchronised its stream: the result is there)
    assert (d_match.cpu().numpy() == exp["match"]).all() and (counts == exp["counts"]).all()


# ---- errors ---------------------------------------------------------------------------------------------

def test_bad_read_byte_names_the_smallest_read_and_writes_nothing(ctx, dev_input):
    import umi_collapse_rs_amd as umi
    wl, reads, _ = dev_input
    bad = reads.copy()
    for r, b, ch in ((2900, 3, ord("x")), (1234, 21, ord("a")), (1234, 5, 0), (2047, 0, ord("n"))):
        bad[r * 22 + b] = ch
    with pytest.raises(umi.UmiHipError) as e:
        device_call(ctx, bad, 22, wl, 2, 1)
    assert e.value.code == umi._lib.UMI_ERR_CHAR
    assert "Unknown character in UMI sequence: 0 (read 1234)" in str(e.value)
    # the outputs as they were: the same call, its outputs looked at after the refusal
    import torch
    n = len(bad) // 22
    outs = [torch.full((len(bad),), 0x5A, dtype=torch.uint8, device="cuda:0"),
            torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0"),
            torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda:0"),
            torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda:0")]
    d_in = dev(bad)
    with pytest.raises(umi.UmiHipError):
        ctx.correct_umis_device(d_in.data_ptr(), n, 22, wl, 2, 1, outs[0].data_ptr(), outs[1].data_ptr(),
                                outs[2].data_ptr(), outs[3].data_ptr())
    torch.cuda.synchronize()
    assert (outs[1].cpu().numpy() == 0x5A5A5A5A).all()
    for t in (outs[0], outs[2], outs[3]):
        assert (t.cpu().numpy() == 0x5A).all()
    # the host form: the same verdict, its arrays untouched (the wrapper's are zero-filled)
    with pytest.raises(umi.UmiHipError) as e:
        ctx.correct_umis(bad, 22, wl, 2, 1)
    assert e.value.code == umi._lib.UMI_ERR_CHAR and "(read 1234)" in str(e.value)
    # and the context is as good as before
    same(ctx.correct_umis(reads, 22, wl, 2, 1), dev_input[2])


def test_bad_whitelist_byte(ctx, dev_input):
    import umi_collapse_rs_amd as umi
    wl, reads, _ = dev_input
    bad = wl.copy()
    bad[7 * 22 + 4] = ord("N")
    with pytest.raises(umi.UmiHipError) as e:
        ctx.correct_umis(reads, 22, bad, 2, 1)
    assert e.value.code == umi._lib.UMI_ERR_CHAR and "Unknown character in whitelist: 78 (entry 7)" in str(e.value)


def test_argument_errors_with_a_context(ctx, dev_input):
    import umi_collapse_rs_amd as umi
    wl, reads, _ = dev_input
    for kw in (dict(max_mismatches=-1), dict(min_distance=-1)):
        with pytest.raises(umi.UmiHipError) as e:
            ctx.correct_umis(reads, 22, wl, **kw)
        assert e.value.code == umi._lib.UMI_ERR_ARG
    with pytest.raises(umi.UmiHipError) as e:
        ctx.correct_umis(reads, 22, np.zeros(0, np.uint8))
    assert e.value.code == umi._lib.UMI_ERR_ARG
    with pytest.raises(umi.UmiHipError) as e:
        ctx.correct_umis(np.tile(np.frombuffer(b"A" * 86, np.uint8), 4), 86, ["C" * 86])
    assert e.value.code == umi._lib.UMI_ERR_ARG


# ---- other contexts -------------------------------------------------------------------------------------

def test_while_a_deferred_call_is_out(ctx, dev_input):
    """umi_dedup_batch_device_begin leaves a call out (every position the fused kernel's); the correction
    lets it end first, and its result is still handed out, and right, afterwards"""
    import torch
    import oracle as orc
    from umi_collapse_rs_amd import synth
    pos, bases = synth.molecule_reads(seed=31, n_positions=2000, reads_per_position=25, umi_len=12, err=0.02)
    st = synth.stage(pos, synth.bases_to_keys(bases))
    keys, freq, off = (np.ascontiguousarray(st["keys"], np.uint64), np.ascontiguousarray(st["freq"], np.int32),
                       np.ascontiguousarray(st["bucket_off"], np.uint64))
    assert np.diff(off.astype(np.int64)).max() <= 128
    okept, oroot, _ = orc.dedup_batch(keys, None, freq, off, 12, 1)
    t_keys, t_freq = dev(keys.view(np.int64)), dev(freq)
    t_kept = torch.zeros(len(keys), dtype=torch.uint8, device="cuda:0")
    t_root = torch.zeros(len(keys), dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    ctx.dedup_batch_device_begin(t_keys.data_ptr(), 0, t_freq.data_ptr(), off, 12, t_kept.data_ptr(), t_root.data_ptr(),
                                 k=1, stream=s.cuda_stream)
    wl, reads, exp = dev_input
    same(ctx.correct_umis(reads, 22, wl, 2, 1), exp)
    same(device_call(ctx, reads, 22, wl, 2, 1), exp)
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all()
    assert (t_root.cpu().numpy().view(np.uint32) == oroot).all()
    assert stats["n_kept"] == int(okept.sum()) and stats["n_umis"] == len(keys)


def test_multi_device_context_uses_its_first_device(dev_input):
    import umi_collapse_rs_amd as umi
    wl, reads, exp = dev_input
    c = umi.Context([0, 0])
    try:
        same(c.correct_umis(reads, 22, wl, 2, 1), exp)
        same(device_call(c, reads, 22, wl, 2, 1), exp)
    finally:
        c.close()
