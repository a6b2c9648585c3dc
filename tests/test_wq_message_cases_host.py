"""tests/wq_message_cases.py on the host: the case table covers every form the wq kernels take (stated here from the basis count alone,
not through the library's own rule), the edge lists are what they claim, the f32 restatement of every case sits within half of the bound
the GPU test uses, and the comparison has power: the f64 reference with one value-only defect moves by at least 10 x that bound."""
import numpy as np
import pytest
import torch

from tests import wq_message_cases as wc

POWER = 10.0
MAIN = wc.MUL_MAIN


def _ks(B):
    """exact-f32 tail steps of a wq record: the basis functions from the seventeenth on and the bias column are the tail; one value
    -> 1, up to five -> 3 (the bf16 tail block), more -> two per step and never fewer than 4 steps"""
    tail = max(B - 16, 0) + 1
    return 1 if tail <= 1 else 3 if tail <= 5 else max(4, (tail + 1) // 2)


def _record_floats(B):
    return 40 if B <= 23 else 48          # include/xeq.h, xeq_message_wq_record_floats_for


def _main(rbf_kind):
    return {B for mul, B, k, _ in wc.TABLE if mul == MAIN and k == rbf_kind}


def test_the_step_rule_restated_here():
    assert [_ks(B) for B in range(1, 32)] == [1] * 16 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 7, 8, 8]


def test_table_reaches_every_tail_form_and_record_width():
    counts = _main("bessel")
    assert {_ks(B) for B in counts} == {1, 3, 4, 5, 6, 7, 8}
    assert {_record_floats(B) for B in counts} == {40, 48}
    for lo, hi in ((16, 17), (20, 21), (23, 24)):
        assert lo in counts and hi in counts and _ks(lo) != _ks(hi)
    assert {1, 7, 8, 9, 15, 16, 17, 20, 21, 22, 23, 24, 25, 27, 28, 29, 30, 31} <= counts
    assert {8, 18, 19} <= _main("gaussian") and 23 in (_main("expnorm") | _main("expbern"))
    for mul in ((32, 0, 0), (32, 32, 0), (32, 0, 32), (64, 64, 64), (160, 96, 64), (256, 32, 32)):
        got = {B for m, B, k, c in wc.TABLE if m == mul}
        assert got >= {8, 20, 22, 26} and {_ks(B) if _ks(B) <= 4 else 8 for B in got} == {1, 3, 4, 8}   # the instantiated step counts
    assert len(set(wc.TABLE)) == len(wc.TABLE)
    assert len({wc.case_id(*row) for row in wc.TABLE}) == len(wc.TABLE)


def test_table_holds_both_sides_of_the_filter_gradient_limits():
    """the matrix-core filter-gradient kernel is admitted for Bessel 12 .. 27 and Gaussian 8 .. 18"""
    assert {11, 12, 27, 28} <= _main("bessel") and {18, 19} <= _main("gaussian") and 8 in _main("gaussian")


# ----------------------------------------------------------------------------------------------------------------- edge lists
@pytest.mark.parametrize("kind", wc.LIST_KINDS)
def test_every_list_kind_has_the_degrees_it_claims(kind):
    el = wc.edge_list(kind)
    n = el.n_nodes
    assert n == 69 and (el.n_edges == 1365 or kind == "symmetric")
    walked = {"directed": [el.c_rowptr], "transpose": [el.n_rowptr], "shuffled": [el.c_rowptr], "symmetric": [el.c_rowptr, el.n_rowptr]}[kind]
    for rowptr in walked:
        seg = np.diff(rowptr)
        assert rowptr.dtype == np.int32 and rowptr[0] == 0 and rowptr[-1] == el.n_edges
        assert {15, 16, 17, 32, 33} <= set(seg.tolist())                  # shorter than, equal to and longer than a 32-row tile
        assert seg[64:68].tolist() == [2, 3, 4, 5]                         # every residue of the quad padding, on consecutive rows
        assert {int(s) % 4 for s in seg} == {0, 1, 2, 3}
        assert seg[-1] == 0 and all(seg[k] == 0 for k in wc.ISOLATED)      # isolated: inside and at the end
    assert (el.c_perm is None) == (kind in ("directed", "symmetric")) and el.n_perm is not None
    assert len(set((el.edge_index[0] * n + el.edge_index[1]).tolist())) == el.n_edges and np.all(el.edge_index[0] != el.edge_index[1])
    for key, rowptr, perm in ((el.edge_index[0], el.c_rowptr, el.c_perm), (el.edge_index[1], el.n_rowptr, el.n_perm)):
        order = np.arange(el.n_edges) if perm is None else perm
        assert sorted(order.tolist()) == list(range(el.n_edges))
        for i in range(n):
            assert np.all(key[order[rowptr[i]:rowptr[i + 1]]] == i)


def test_edge_vectors_cutoff_skin_and_mirror():
    for kind in wc.LIST_KINDS:
        el = wc.edge_list(kind)
        vec, beyond = wc.edge_vectors(el)
        ei, d = el.edge_index, vec.norm(dim=1).numpy()
        assert torch.equal(vec, vec.float().double())
        at = (ei[0] == wc.CUTOFF_NODE) | (ei[1] == wc.CUTOFF_NODE)
        skin = ((ei[0] == wc.SKIN_NODE) | (ei[1] == wc.SKIN_NODE)) & ~at
        assert at.sum() >= 1 and np.all(d[at] == wc.CUTOFF) and skin.sum() >= 1 and np.all(d[skin] > wc.CUTOFF)
        live = ~(at | skin)
        assert np.array_equal(beyond.numpy(), ~live) and d[live].min() > 0.69 and d[live].max() < wc.CUTOFF
        # a node whose every walked edge is dead (forward: CUTOFF_NODE and SKIN_NODE are centers of dead edges only)
        assert all(not live[ei[0] == k].any() for k in (wc.CUTOFF_NODE, wc.SKIN_NODE))
    el = wc.edge_list("symmetric")
    vec, _ = wc.edge_vectors(el)
    rev = el.n_perm
    assert np.array_equal(rev[rev], np.arange(el.n_edges)) and torch.equal(vec[torch.tensor(rev).long()], -vec)   # what the mirror walk assumes


def test_bt_layout_round_trip():
    mul, n = (32, 0, 32), 3
    x = torch.arange(n * (32 + 160), dtype=torch.float64).reshape(n, -1)
    flat = wc.to_bt(x, mul)
    assert torch.equal(wc.from_bt(flat, mul, n), x)
    # addr(n, u, m) of block l = 2: N base + (n 5 + m) mul + u, base = mul_0
    node, u, m = 2, 7, 3
    assert flat[n * 32 + (node * 5 + m) * 32 + u] == x[node, 32 + u * 5 + m]


def test_list_order_does_not_move_the_reference():
    a, b = wc.message_case(MAIN, 20), wc.message_case(MAIN, 20, list_kind="shuffled")
    perm = np.random.default_rng(22).permutation(a.edges.n_edges)
    assert np.array_equal(a.edges.edge_index[:, perm], b.edges.edge_index)
    for k in wc.OUTPUTS + wc.PARAM_GRADS[:3]:
        want = a.ref[k][torch.tensor(perm)] if k == "grad_vec" else a.ref[k]
        assert float((b.ref[k] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), k


# ------------------------------------------------------------------------------------------- the bound has a factor in hand
@pytest.mark.parametrize("row", wc.TABLE, ids=[wc.case_id(*r) for r in wc.TABLE])
def test_f32_restatement_within_half_the_bound(row):
    c = wc.message_case(*row)
    worst = {}
    for names, tol in ((wc.OUTPUTS, wc.TOL_OUT), (wc.PARAM_GRADS, wc.TOL_PARAM)):
        for k in names:
            if c.ref[k] is None:
                assert k == "grad_p1" and c.p1 is None
                continue
            assert torch.isfinite(c.ref[k]).all() and torch.isfinite(c.ref32[k]).all(), k
            err = float((c.ref32[k].double() - c.ref[k]).abs().max())
            worst[k] = err / (tol * max(1.0, float(c.ref[k].abs().max())))
            assert wc.bound(c.ref[k], c.ref32[k], tol) == tol * max(1.0, float(c.ref[k].abs().max()))   # the widening takes no effect
    print(c.id, {k: f"{v:.3f}" for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst
    assert float(c.ref["grad_vec"][c.beyond].abs().max()) == 0.0 and float(c.ref32["grad_vec"][c.beyond].abs().max()) == 0.0


@pytest.mark.parametrize("list_kind", wc.LIST_KINDS[1:])
@pytest.mark.parametrize("B", wc.PER_INSTANTIATION)
def test_f32_restatement_within_half_the_bound_other_lists(B, list_kind):
    c = wc.message_case(MAIN, B, list_kind=list_kind)
    for k in wc.OUTPUTS:
        err = float((c.ref32[k].double() - c.ref[k]).abs().max())
        assert err <= 0.5 * wc.TOL_OUT * max(1.0, float(c.ref[k].abs().max())), (k, err)


# ------------------------------------------------------------------------------------------------------------------- power
@pytest.mark.parametrize("B", [8, 16, 17, 20, 21, 23, 24, 26, 29, 31])
def test_power_of_the_comparison(B):
    """A dropped bias column (the tail position behind the last basis function), a dropped last basis function and a dropped
    seventeenth one (the first tail position) each move every output that depends on the filter by at least POWER x its bound."""
    c = wc.message_case(MAIN, B)
    names = tuple(k for k in wc.OUTPUTS if k not in ("grad_s", "grad_x"))      # (the residual path does not see the filter)
    defects = {"bias column dropped": dict(b=torch.zeros_like(c.b))}
    for col, what in ((B - 1, "last basis function dropped"), (16, "seventeenth basis function dropped")):
        if col < B:
            W = c.W.clone()
            W[:, col] = 0.0
            defects[what] = dict(W=W)
    for what, kw in defects.items():
        bad = wc.message_eval(c, torch.float64, **kw)
        moved = {k: float((bad[k] - c.ref[k]).abs().max()) / wc.bound(c.ref[k], c.ref32[k], wc.TOL_OUT) for k in names}
        assert all(v >= POWER for v in moved.values()), (what, moved)
        # ... and the filter gradients see it through dL/dp0 (dL/dW and dL/db do not depend on W and b)
        moved_p = float((bad["grad_p0"] - c.ref["grad_p0"]).abs().max()) / wc.bound(c.ref["grad_p0"], c.ref32["grad_p0"], wc.TOL_PARAM)
        assert what == "bias column dropped" or moved_p >= POWER, (what, moved_p)
