"""What tests/pair_run_inputs.py builds, from the models alone: exactly RUNS at exactly START in sorted order, for
the buckets of a pair and for the entries of a UMI, in the given and in the permuted order; and that the inputs give
every payload something to carry."""
import numpy as np
import pytest

import gene_model
import pair_run_inputs as pri
import saturation_model
import stats_model
import velocity_model as vm


def test_the_layout_is_the_one_the_edges_need():
    assert pri.N_ELEMENTS == 1536 and len(pri.RUNS) == 11
    start, end = np.array(pri.START), np.array(pri.START) + np.array(pri.RUNS)
    lane = lambda p: p % 64
    assert (lane(start[0]), lane(end[0] - 1)) == (0, 63) and pri.RUNS[0] == 64  # exactly a wave
    assert lane(start[1]) == 0 and pri.RUNS[1] == 1                              # a single at lane 0
    assert lane(end[2] - 1) == 63 and lane(start[2]) != 0                        # ends on lane 63
    assert start[3] // 64 + 1 == (end[3] - 1) // 64                              # crosses one wave edge
    assert pri.RUNS[5] == 1 and start[5] % 256 == 255                            # a single on a block's last lane
    assert start[6] % 256 == 0 and pri.RUNS[6] == 128                            # two whole waves from a block edge on
    assert start[7] < 512 < end[7] - 1                                           # crosses the block edge at 512
    for r in (8, 10):                                                            # whole middle waves
        assert (end[r] - 1) // 64 - start[r] // 64 >= 3
    assert pri.RUNS[9] == 3
    assert all(start[8] <= at < end[8] and 33 <= size <= 40 for at, size in pri.BIG.items()) and len(pri.BIG) == 5


@pytest.mark.parametrize("permuted", [False, True])
def test_matrix_runs_and_positions(permuted):
    m = pri.matrix_case(permuted)
    nb = len(m["off"]) - 1
    assert nb == pri.N_ELEMENTS and (np.diff(m["off"].astype(np.int64)) > 0).all()  # no empty bucket: a position is a bucket
    # a bucket counted as one molecule: the model's molecules are the runs' lengths, in sorted order
    row, col, length, _ = gene_model.count_model(np.ones(nb, np.uint8), np.ones(nb, np.int32), np.arange(nb + 1), m["row"], m["col"])
    assert tuple(int(x) for x in length) == pri.RUNS
    assert tuple(int(x) for x in np.concatenate([[0], np.cumsum(length)[:-1]])) == pri.START
    key = (col.astype(np.int64) << 2) | row
    assert (key == np.arange(len(pri.RUNS))).all() and int(m["row"].max()) < pri.N_ROWS and int(m["col"].max()) < pri.N_COLS
    # the sort is stable: sorted position p holds the p-th bucket of its pair in the given order
    order = np.argsort((m["col"].astype(np.int64) << 2) | m["row"], kind="stable")
    sizes = np.diff(m["off"].astype(np.int64))[order]
    big = {int(p): int(sizes[p]) for p in np.flatnonzero(sizes > 3)}
    assert sorted(big.values()) == sorted(pri.BIG.values()) and sizes.min() == 1
    assert all(pri.START[8] <= p < pri.START[9] for p in big) and (permuted or big == pri.BIG)  # (inside the 257-run)
    assert permuted == bool((np.diff(order) < 0).any())


@pytest.mark.parametrize("permuted", [False, True])
def test_matrix_payloads(permuted):
    m = pri.matrix_case(permuted)
    _, _, molecules, reads = gene_model.count_model(m["kept"], m["freq"], m["off"], m["row"], m["col"])
    assert len(molecules) == len(pri.RUNS) and (molecules > 0).all() and int(molecules.sum()) == int(np.count_nonzero(m["kept"]))
    assert int(reads[10]) > 700 and int(molecules[1]) <= 3
    v = vm.velocity_model(m["read_entry"], m["read_class"], m["kept"], m["root"], m["off"], m["row"], m["col"])
    assert (v[2].astype(np.int64) + v[3] + v[4] == molecules).all() and min(int(v[k].sum()) for k in (2, 3, 4)) > 100
    curve = saturation_model.saturation_model(m["sat_entry"], m["kept"], m["root"], m["off"], m["row"], m["col"], pri.N_COLS,
                                              pri.SAT_LEVELS, 0, np.ones(pri.N_COLS, np.uint8))
    pairs = [int(x) for x in curve[:, 2]]
    # pairs turn up at several depths, and not every pair has a read at all: the minimum decides, run by run
    assert len(set(pairs)) >= 3 and 0 < pairs[0] < pairs[-1] <= len(pri.RUNS) and (curve[:, 5] == curve[:, 2]).all()
    assert int(curve[-1, 1]) < 60  # so few molecules that a run's level lies in one or two of its buckets


def test_both_orders_are_one_matrix():
    a, b = pri.matrix_case(False), pri.matrix_case(True)
    for x, y in zip(gene_model.count_model(a["kept"], a["freq"], a["off"], a["row"], a["col"]),
                    gene_model.count_model(b["kept"], b["freq"], b["off"], b["row"], b["col"])):
        assert (x == y).all()


@pytest.mark.parametrize("permuted", [False, True])
def test_stats_runs_and_positions(permuted):
    keys, freq, kept, root, off, L = pri.stats_case(permuted)
    assert L == 12 and stats_model.n_words_of(L) == 1 and len(keys) == pri.N_ELEMENTS == int(off[-1])
    exp = stats_model.stats_model(keys, freq, kept, root, off, L, hist_bins=64)
    assert tuple(int(x) for x in exp["times_pre"]) == pri.RUNS  # (the table is in ascending key order: the sorted order)
    assert (exp["reads_pre"] >= exp["times_pre"]).all() and 0 < int(exp["times_post"].sum()) < pri.N_ELEMENTS
    assert int(exp["reads_post"].sum()) == int(np.asarray(freq).sum())
    sizes = np.diff(off.astype(np.int64))
    assert len(sizes) == 700 and sizes.min() == 1 and sizes.max() == 11 and (sizes > 8).sum() >= 2
    for b in range(len(sizes)):  # a bucket holds a UMI once
        assert len(set(keys[int(off[b]):int(off[b + 1])].tolist())) == sizes[b]
