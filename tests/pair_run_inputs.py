"""One layout of runs for the four users of the shared run scan (csrc/umihip_pair_table.h: WaveRuns) --
umi_count_matrix, umi_velocity_matrix, umi_saturation_curve and the per-UMI table of umi_dedup_stats.

In sorted order the runs are RUNS elements long, 1,536 elements in all, so with a lane per element, waves of 64 and
blocks of 256 there is: a run that is exactly a wave (head at lane 0, end at lane 63); a single at lane 0; a run
ending on lane 63; one crossing one wave edge; one ending short of a block's last lane; a single on it (position
255); two whole waves starting on a block edge; a run crossing the block edge at 512; runs with whole middle waves
that hold neither their head nor their end (257, 700); a short tail.

For the three matrix calls an element is a bucket and a run the buckets of one (column, row) pair: pair ids ascend
with the run, so the sorted position of every run is START[r].  A bucket has 1 to 3 entries, except BIG buckets of
33 to 40 entries (a wave's in the bucket walk, the others a lane's) inside the 257-run.  For the per-UMI table an
element is an entry and a run the entries of one UMI, spread over buckets.  Either input comes in that order and
with its buckets permuted."""
import functools

import numpy as np

import stats_model
import velocity_model as vm

RUNS = (64, 1, 63, 65, 62, 1, 128, 192, 257, 3, 700)
START = tuple(int(x) for x in np.concatenate([[0], np.cumsum(RUNS)[:-1]]))
N_ELEMENTS = sum(RUNS)
N_ROWS, N_COLS = 4, 3  # pair r is (col, row) = (r // N_ROWS, r % N_ROWS): the sort key col << 2 | row is r
BIG = {START[8] + 10: 33, START[8] + 70: 35, START[8] + 130: 37, START[8] + 200: 39, START[8] + 250: 40}  # position: entries
SAT_LEVELS = 4
UMI_LEN = 12


def run_of_position():
    return np.repeat(np.arange(len(RUNS)), RUNS)


def _entries(rng, sizes):
    """kept, freq, root over buckets of these sizes: a bucket's first entry is kept, the others with probability 0.6
    and rooted at the first otherwise (umi_dedup_stats' contract for root[], which the other calls accept)"""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    first = np.repeat(off[:-1], sizes)
    kept = (rng.random(n) < 0.6) | (np.arange(n) == first)
    root = np.where(kept, np.arange(n), first)
    return kept.astype(np.uint8), rng.integers(1, 10, n).astype(np.int32), root.astype(np.uint32), off


def _permute(rng, permuted, off, per_bucket, per_entry, root):
    """the buckets in another order, their entries moving with them: (off, per_bucket, per_entry, root, new index of
    every old entry)"""
    nb = len(off) - 1
    order = rng.permutation(nb) if permuted else np.arange(nb)
    sizes = np.diff(off)[order]
    new_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    old = np.concatenate([np.arange(off[b], off[b + 1]) for b in order])  # old index of every new entry
    new = np.empty(len(old), np.int64)
    new[old] = np.arange(len(old))
    return (new_off.astype(np.uint64), [a[order] for a in per_bucket], [a[old] for a in per_entry],
            new[root[old].astype(np.int64)].astype(np.uint32), new)


@functools.lru_cache(maxsize=None)
def matrix_case(permuted):
    """dict(kept, freq, root, off, row, col, read_entry, read_class, sat_entry): read_entry / read_class are about three
    reads an entry for umi_velocity_matrix; sat_entry are one to four reads a run for umi_saturation_curve -- so few
    that a pair's level is the level of one or two buckets somewhere in its run, which the minimum has to carry
    there"""
    rng = np.random.default_rng(20)
    run = run_of_position()
    sizes = rng.integers(1, 4, N_ELEMENTS)
    for at, size in BIG.items():
        sizes[at] = size
    kept, freq, root, off = _entries(rng, sizes)
    n = int(off[-1])
    row, col = (run % N_ROWS).astype(np.uint32), (run // N_ROWS).astype(np.uint32)
    read_entry = rng.permutation(np.repeat(np.arange(n), rng.integers(0, 6, n))).astype(np.uint32)
    read_class = rng.integers(0, 5, len(read_entry)).astype(np.uint8)
    entry_run = np.repeat(run, sizes)
    sat = [rng.choice(np.flatnonzero(entry_run == r), min(int(rng.integers(1, 5)), int((entry_run == r).sum())), replace=False)
           for r in range(len(RUNS))]
    sat_entry = rng.permutation(np.concatenate(sat + [[e for at in BIG for e in range(off[at] + 30, off[at] + 33)]]))
    off, (row, col), (kept, freq), root, new = _permute(rng, permuted, off, [row, col], [kept, freq], root)
    read_entry, sat_entry = new[read_entry].astype(np.uint32), new[sat_entry].astype(np.uint32)
    for reads in (read_entry, sat_entry):
        reads[rng.random(len(reads)) < 0.1] = vm.UNSTAGED
    return dict(kept=kept, freq=freq, root=root, off=off, row=row, col=col, read_entry=read_entry, read_class=read_class,
                sat_entry=sat_entry)


@functools.lru_cache(maxsize=None)
def stats_case(permuted):
    """(keys, freq, kept, root, off, UMI_LEN): entry k of run r lies in bucket k, so a bucket holds every UMI at most
    once; 700 buckets of 1 to 11 entries (more than 8: a wave's in the distance kernels)"""
    rng = np.random.default_rng(21)
    umis = set()
    while len(umis) < len(RUNS):
        umis.add("".join("ACGT"[x] for x in rng.integers(0, 4, UMI_LEN)))
    keys = np.sort(stats_model.encode(sorted(umis), UMI_LEN))  # (one word a key: run r has the r-th smallest)
    sizes = np.array([sum(1 for length in RUNS if length > k) for k in range(max(RUNS))])
    entry_run = np.concatenate([[r for r, length in enumerate(RUNS) if length > k] for k in range(max(RUNS))])
    kept, freq, root, off = _entries(rng, sizes)
    off, _, (kept, freq, entry_run), root, _ = _permute(rng, permuted, off, [], [kept, freq, entry_run], root)
    return keys[entry_run], freq, kept, root, off, UMI_LEN
