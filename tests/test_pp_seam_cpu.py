"""The block-step fixture's contract (tests/pp_ref.py on tests/seam_data.py),
checked without a GPU, and the fp32 C oracle's block step alone against the
float64 one: at most a quarter of the 1e-4 bar in both error measures, so a
GPU block or prediction that misses the bar against float64 in
test_pp_seam_gpu.py is the kernel's doing, not the restatement's.
"""
import numpy as np
import pytest

import pp_ref as P
import seam_data as S


def test_block_list_coverage():
    P.check_coverage()
    assert set(P.BLOCKS) == set(P.DIMS) == set(P.PADDED)
    for d, Dp in P.PADDED.items():
        assert Dp >= d and (Dp == d or Dp % 32 == 0)
    # every TB at its lower and its upper width
    widths = {e - s for bl in P.BLOCKS.values() for s, e in bl}
    for tb in (1, 2, 3, 4):
        assert {32 * (tb - 1) + 1, 32 * tb} <= widths
    # the three width-1 blocks the oracle itself misses the cap on stay out
    for d, s, e in ((20, 19, 20), (256, 255, 256), (1000, 999, 1000)):
        assert (s, e) not in P.BLOCKS[d]
    # a check that can fail: a list without TB = 3 is refused
    with pytest.raises(AssertionError):
        P.check_coverage({100: tuple(b for b in P.BLOCKS[100] if P.tile_count(b[1] - b[0]) != 3)},
                         P.PADDED)


@pytest.mark.parametrize("key", ["ials_user", "ials_item"])
def test_rating_index_is_the_file_position(key):
    p = P.pp_case(key, 8)
    c = p.c
    ent, oth = S._pairs(S.seam_data())
    users_file, items_file = (ent, oth) if c.seam == "user" else (oth, ent)
    for rix, ptr, col, rows_file, cols_file in ((p.urix, c.up, c.uc, users_file, items_file),
                                                (p.irix, c.ip, c.ic, items_file, users_file)):
        assert sorted(rix.tolist()) == list(range(p.nnz))  # a permutation
        np.testing.assert_array_equal(col, cols_file[rix])
        np.testing.assert_array_equal(np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)),
                                      rows_file[rix])
    assert p.rix is (p.urix if c.seam == "user" else p.irix)
    ident = np.arange(p.nnz)
    if c.seam == "user":  # the file is sorted by seam entity
        np.testing.assert_array_equal(p.urix, ident)
        assert (p.irix != ident).any()
    else:  # as_items: the user side's index is a non-identity permutation too
        assert (p.urix != ident).any()
        np.testing.assert_array_equal(p.irix, ident)


@pytest.mark.parametrize("key", P.KEYS)
def test_fixture_holds_what_the_block_kernel_trips_on(key):
    p = P.pp_case(key, 8)
    c = p.c
    for h in P.HISTORY_LENGTHS:
        assert (c.h == h).any(), h
    assert c.h.max() == 640 and (c.h == 0).sum() >= 3
    hists = [c.col[c.ptr[e]:c.ptr[e + 1]] for e in p.live]
    assert sum(len(np.unique(x)) < len(x) for x in hists) >= 3  # repeated ids
    assert any(0 in x for x in hists) and any(c.n_other - 1 in x for x in hists)
    if c.kind == 1:
        assert (c.entity_weight[p.live] == 0).sum() >= 5
    if c.kind == 2:
        assert c.labels.count("nu0") == 1
        e = c.labels.index("nu0")
        assert c.h[e] > 0 and (c.other_weight[c.col[c.ptr[e]:c.ptr[e + 1]]] == 0).all()
        inside = [x for x in hists if (c.other_weight[x] == 0).any() and (c.other_weight[x] > 0).any()]
        assert len(inside) >= 10  # nu = 0 rows inside a history


def _oracle_figures(key, dim, blocks):
    """Per step: (block errors, prediction errors, relative residual error)
    of the oracle against float64."""
    p = P.pp_case(key, dim)
    out = []
    for ref, orc in zip(P.reference(key, dim, blocks), P.oracle_steps(key, dim, blocks)):
        assert orc.rc == 0
        out.append((P.block_errors(p, ref, orc.E), P.pred_errors(p, ref, orc.pred),
                    abs(orc.residual - ref.residual) / ref.residual))
    return p, out


@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_oracle_block_step_within_a_quarter_of_the_bar(case):
    """Measured on this fixture: block error <= 2.0e-6 and prediction error
    <= 1.1e-6 for widths >= 5; width 1 up to 1.9e-5 in the block; residual
    <= 9.4e-7 relative."""
    key, dim, blk = case
    p, figs = _oracle_figures(key, dim, blk)
    (eb, ep, er), = figs
    print(f"pp oracle vs float64: {P.case_id(case)} block {P.worst(p, eb)} pred {P.worst(p, ep)} "
          f"residual {er:.2e}")
    assert not P.offenders(p, eb, P.ORACLE_CAP), P.offenders(p, eb, P.ORACLE_CAP)
    assert not P.offenders(p, ep, P.ORACLE_CAP), P.offenders(p, ep, P.ORACLE_CAP)
    assert er <= 1e-5
    # outside the block and on idle rows the restatements leave the start rows
    c = p.c
    ref, = P.reference(key, dim, blk)
    orc, = P.oracle_steps(key, dim, blk)
    s, e = blk
    for E in (ref.E, orc.E):
        np.testing.assert_array_equal(E[:, :s], c.E[:, :s])
        np.testing.assert_array_equal(E[:, e:], c.E[:, e:])
        np.testing.assert_array_equal(E[c.h == 0], c.E[c.h == 0])


@pytest.mark.parametrize("key", P.TWO_STEP_KEYS)
def test_oracle_two_consecutive_blocks(key):
    """[0,65) then [65,100) at d = 100: the second step consumes the first
    step's predictions; the oracle stays under the cap after both."""
    p, figs = _oracle_figures(key, 100, P.TWO_STEP)
    for (s, e), (eb, ep, er) in zip(P.TWO_STEP, figs):
        print(f"pp oracle two-step {key} [{s},{e}): block {P.worst(p, eb)} pred {P.worst(p, ep)} "
              f"residual {er:.2e}")
        assert not P.offenders(p, eb, P.ORACLE_CAP)
        assert not P.offenders(p, ep, P.ORACLE_CAP)
        assert er <= 1e-5
    # the sequence is not two independent steps: the second one from the
    # start predictions lands elsewhere
    first, second = P.reference(key, 100, P.TWO_STEP)
    alone, = P.reference(key, 100, P.TWO_STEP[1])
    rel = np.linalg.norm(second.delta - alone.delta) / np.linalg.norm(second.delta)
    assert rel > 1e-2, rel


@pytest.mark.parametrize("dim", P.DIMS)
@pytest.mark.parametrize("key", ["ials_user", "ials_item"])
def test_oracle_predict(key, dim):
    """The oracle's serial fp32 dot product against float64: the plain bound
    (Dp + 1) 2^-24 sum |x_i u_i|."""
    p = P.pp_case(key, dim)
    ref, mag = P.pred0(p), P.pred0_magnitude(p)
    out = P.oracle_pred0(key, dim)
    assert (np.abs(out - ref) <= (dim + 1) * 2.0 ** -24 * mag).all()
    assert (mag > 0).all()
