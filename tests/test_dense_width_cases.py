"""The cases of tests/dense_width_cases.py on their formulas and the oracle alone, without a GPU: every register width
NT = 4 .. 64 and every depth class of K1w's LDS ring occurs, each (model, variant, unit_rows) names its kernel or its
refusal, and every case is worth running -- the oracle accepts a fair share of the proposals from the first sweep on, and
every 64-variable slot holds a variable that ends elsewhere than it started, so a width that drops a slot cannot pass
tests/test_gpu_dense_widths.py.  The large-model cases (tests/test_gpu_dense_xl_edges.py): their shapes are the group, column
and chunk edges they are named for, the cold replicas of xl_model() do what the dead-range case needs of them."""
import numpy as np
import pytest

import dense_width_cases as dc


def test_every_width_occurs():
    assert [dc.width(n) for n in dc.FULL] == list(dc.WIDTHS) and len(dc.WIDTHS) == 16
    for n in dc.FULL:                                    # "full": every slot of the width in use, the last one ragged
        assert dc.slots(n) == dc.width(n) and n % 64 == 27
    assert {n: (dc.width(n), dc.slots(n), n % 64) for n in dc.EXTRA} == {
        1281: (24, 21, 1), 2816: (44, 44, 0), 2817: (48, 45, 1), 3841: (64, 61, 1), 4096: (64, 64, 0)}
    assert dc.width(1) == 4 and dc.width(256) == 4 and dc.width(257) == 8 and dc.width(4096) == 64
    assert dc.R % 4 != 0 and dc.R % 16 != 0 and dc.R > 16          # a ragged K1 block, a ragged second K1w workgroup
    assert len(dc.BETAS) == 5 and len(dc.SIZES) == 21


def test_every_ring_depth_class_occurs():
    """WgCfg<NT,GR>::U restated: the depth per width, its classes (capped, fitting, the minimum of 3, refused), and the
    expected names / refusals."""
    depth4 = {nt: dc.ring_depth(nt, 4) for nt in dc.WIDTHS}
    depth2 = {nt: dc.ring_depth(nt, 2) for nt in dc.WIDTHS}
    print("U at GR = 4:", depth4)
    print("U at GR = 2:", depth2)
    assert depth4 == {4: 17, 8: 17, 12: 13, 16: 9, 20: 7, 24: 6, 28: 5, 32: 4, 36: 4, 40: 3, 44: 3, 48: 3, 52: 3, 56: 2, 60: 2, 64: 2}
    assert depth2 == {4: 32, 8: 32, 12: 26, 16: 19, 20: 15, 24: 13, 28: 11, 32: 9, 36: 8, 40: 7, 44: 7, 48: 6, 52: 6, 56: 5, 60: 5, 64: 4}
    assert [nt for nt in dc.WIDTHS if dc.ring_class(nt, 4) == "cap"] == [4, 8]
    assert [nt for nt in dc.WIDTHS if dc.ring_class(nt, 2) == "cap"] == [4, 8]
    assert [nt for nt in dc.WIDTHS if dc.ring_class(nt, 4) == "min"] == [40, 44, 48, 52]
    assert [nt for nt in dc.WIDTHS if dc.ring_class(nt, 4) == "refused"] == [56, 60, 64]
    assert all(dc.ring_ok(nt, 2) for nt in dc.WIDTHS)
    assert [dc.auto_unit_rows(nt) for nt in (52, 56, 60, 64)] == [4, 2, 2, 2]
    sizes = {dc.width(n) for n in dc.SIZES}
    for cls in ("cap", "fit", "min", "refused"):
        assert any(dc.ring_class(nt, 4) == cls for nt in sizes), cls
    # the names: every kernel family at every width it is built for, refusals where it is not
    names = {dc.expected(n, v, u) for n in dc.SIZES for v, u in dc.VARIANTS}
    for nt in dc.WIDTHS:
        assert "k_anneal_dense<%d>" % nt in names and "k_anneal_dense_wg<%d,2>" % nt in names
        assert ("k_anneal_dense_wg<%d,4>" % nt in names) == (nt <= 52)
        assert ("k_anneal_dense_mfma<%d>" % nt in names) == (nt <= 44)
    for n in dc.SIZES:
        nt = dc.width(n)
        assert (dc.expected(n, 2, 4) is None) == (nt >= 56) and (dc.expected(n, 3) is None) == (nt >= 48)
        assert dc.expected(n, 2, 0) == "k_anneal_dense_wg<%d,%d>" % (nt, 2 if nt >= 56 else 4)
    assert dc.expected(2816, 3) == "k_anneal_dense_mfma<44>" and dc.expected(2817, 3) is None
    assert [dc.expected(n, 2, 0) for n in dc.AUTO_SIZES] == ["k_anneal_dense_wg<48,4>", "k_anneal_dense_wg<64,2>"]
    assert dc.AUTO_R >= 32 and len(dc.AUTO_BETAS) == 8 and -(-len(dc.AUTO_BETAS) // dc.AUTO_CHUNK) == 3


@pytest.mark.parametrize("scenario", dc.SCENARIOS)
@pytest.mark.parametrize("n", dc.SIZES)
def test_case_is_not_vacuous_on_the_oracle(n, scenario):
    ref = dc.reference(n, scenario)
    start = dc.oracle(n, scenario, betas=dc.BETAS[:0])[0]
    first = dc.oracle(n, scenario, betas=dc.BETAS[:1])
    share, share1 = ref.accepted / ref.proposals, first[3] / first[2]
    moved = (ref.states != start).any(axis=0)                        # [n]: some replica ends elsewhere than it started
    per_slot = np.add.reduceat(moved, np.arange(0, n, 64))
    print("n = %d (NT = %d) %s: accepted %.3f overall, %.3f in the first sweep; fewest moved variables of a slot %d"
          % (n, dc.width(n), scenario, share, share1, per_slot.min()))
    assert ref.proposals == dc.R * len(dc.BETAS) * n and first[2] == dc.R * n
    assert 0.05 <= share <= 0.60 and share1 >= 0.30
    assert len(per_slot) == dc.slots(n) and per_slot.min() >= 1
    assert ref.states.any(axis=1).all() and not ref.states.all(axis=1).any()
    if scenario == "init":
        assert np.array_equal(start, dc.given_start(n)) and dc.RESYNC < len(dc.BETAS)
    else:
        assert 0.3 < start.mean() < 0.7 or n < 300


@pytest.mark.parametrize("n", dc.AUTO_SIZES)
def test_auto_case_is_not_vacuous_on_the_oracle(n):
    ref = dc.auto_reference(n)
    assert ref.proposals == dc.AUTO_R * len(dc.AUTO_BETAS) * n and 0.05 <= ref.accepted / ref.proposals <= 0.60


def test_large_model_shapes_are_the_edges_they_are_named_for():
    # (blocks, groups, blocks of the last group, variables of the last block, column ranges, ncols exact, K1x chunks)
    assert dc.xl_shape(4160) == (65, 9, 1, 64, 17, False, 2)
    assert dc.xl_shape(4352) == (68, 9, 4, 64, 17, True, 2)
    assert dc.xl_shape(4353) == (69, 9, 5, 1, 18, False, 2)
    assert dc.xl_shape(4608) == (72, 9, 8, 64, 18, True, 2)
    assert dc.xl_shape(8192) == (128, 16, 8, 64, 32, True, 2)
    assert dc.xl_shape(8193) == (129, 17, 1, 1, 33, False, 3)
    assert dc.B1_SIZES == (4160, 4352, 4353, 4608) and dc.B2_SIZES == (8192, 8193)
    assert dc.B3_COUNTS == (64, 65, 257, 512, 513)
    assert [dc.b3_windows(r) for r in (64, 65, 513)] == [[(0, 2), (62, 2), (62, 2)], [(0, 2), (62, 3), (63, 2)],
                                                         [(0, 2), (62, 4), (511, 2)]]
    # B4: the planted ones are where the table says, and nowhere else
    nb = dc.xl_shape(dc.B4_N)[0]
    live = {}
    for r, i in dc.b4_planted():
        assert 128 <= r < 192 and 0 <= i < dc.B4_N
        live.setdefault(i // 64 // dc.XG_GROUP, set()).add(i // 64 % dc.XG_GROUP)
    assert {g: tuple(sorted(b)) for g, b in live.items()} == dc.B4_LIVE
    assert dc.XG_GROUP * 8 + 4 == nb - 1 and (dc.B4_N - 1) // 64 == nb - 1
    planted = dc.b4_planted()
    assert len(set(planted)) == len(planted)
    per_replica = np.bincount([r - 128 for r, _ in planted], minlength=64)
    assert per_replica.min() == 0 and per_replica.max() >= 3            # replicas with no one at all beside busy ones
    betas, init = dc.b4_inputs()
    assert init[64:128].sum() == 0 and init[128:].sum() == len(planted) and 0.45 < init[:64].mean() < 0.55
    assert np.all(betas[64:] == dc.B4_COLD) and betas[0] == 0.05 and betas[63] == pytest.approx(5.0)


def test_cold_replicas_of_the_large_model_do_what_the_dead_range_case_needs():
    """xl_model(4353): from all zeros at beta = 1e4 nothing is accepted; planted ones flip back, one accepted move each, and
    nothing else moves; random starts from beta = 0.05 to 5 accept about half of their proposals.  Then the case itself."""
    n = dc.B4_N
    Qs = dc.xl_model(n)
    assert np.array_equal(Qs, Qs.T) and Qs.diagonal().min() >= 2.0 and Qs.diagonal().max() <= 3.0
    off = Qs[~np.eye(n, dtype=bool)]
    assert 0.019 < np.count_nonzero(off) / off.size < 0.021 and np.abs(off).max() <= 0.5
    cold = np.full(2, dc.B4_COLD)
    zero = dc.xl_oracle(n, 2, cold, init=np.zeros((2, n), dtype=np.uint8), num_sweeps=3)
    assert zero.accepted == 0 and not zero.states.any()
    five = np.zeros((2, n), dtype=np.uint8)
    five[0, [3, 700, 2048, 4000, n - 1]] = 1
    five[1, [0, 63, 64, 4351, 4352]] = 1
    back = dc.xl_oracle(n, 2, cold, init=five, num_sweeps=3)
    assert back.accepted == 10 and not back.states.any()
    hot = dc.xl_oracle(n, 4, np.geomspace(0.05, 5.0, 4), init=dc.xl_start(n, 4), num_sweeps=3)
    print("random starts, beta 0.05 .. 5: accepted %.3f" % (hot.accepted / hot.proposals))
    assert 0.40 < hot.accepted / hot.proposals < 0.65
    # the case: replicas 64 .. 191 end all zero, the planted ones are the only moves of replicas 128 .. 191
    betas, init = dc.b4_inputs()
    ref = dc.b4_reference()
    assert not ref.states[64:].any()
    alone = dc.xl_oracle(n, 64, betas[128:], init=init[128:], num_sweeps=dc.B4_SWEEPS, replica_offset=128)
    assert alone.accepted == len(dc.b4_planted()) and not alone.states.any()
    rest = dc.xl_oracle(n, 64, betas[:64], init=init[:64], num_sweeps=dc.B4_SWEEPS)
    assert ref.accepted == rest.accepted + alone.accepted and np.array_equal(rest.states, ref.states[:64])
    assert 0.40 < rest.accepted / rest.proposals < 0.65
