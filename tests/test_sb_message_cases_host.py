"""tests/sb_message_cases.py on the host: the table reaches every instantiation of the sb kernels on both sides of its limits (stated
here from the basis count alone), the edge lists are what they claim, the reference is the arithmetic of
tests/test_gpu_parity.py::_message_case (restated here line by line, and once more as a loop over the edges), the f32 restatement of
every tensor sits within half of the plain bound -- the widening of ``wq_message_cases.bound`` to 1.5 x err32 takes effect nowhere, for
no forward output, first-order or second-order gradient of any case, so there is no exception to list -- and the comparison has power:
the f64 reference with one value-only defect moves by at least 10 x the bound."""
import math

import numpy as np
import pytest
import torch

from oracle import xpainn_oracle as orc
from tests import sb_message_cases as sc
from tests import wq_message_cases as wc

POWER = 10.0


def _plain(ref, tol):
    return tol * max(1.0, float(ref.abs().max())) if ref.numel() else tol


def _err32_over_plain(c, names, tol):
    """{tensor: err32 / plain bound}; asserts that ``bound`` is the plain bound (the widening takes no effect)"""
    out = {}
    for k in names:
        ref, r32 = c.ref[k], c.ref32[k]
        assert ref.shape == r32.shape and torch.isfinite(ref).all() and torch.isfinite(r32).all(), (c.id, k)
        if ref.numel() == 0:
            continue
        err = float((r32.double() - ref).abs().max())
        out[k] = err / _plain(ref, tol)
        widened = 1.5 * err > _plain(ref, tol)
        assert not widened and wc.bound(ref, r32, tol) == _plain(ref, tol), (c.id, k, err)
    return out


# ---------------------------------------------------------------------------------------------------------------------- table
def test_table_reaches_every_instantiation_and_padded_head():
    main = {B for F, mul, B, k, _ in sc.TABLE if (F, mul) == sc.MAIN and k == "bessel"}
    assert main == set(range(1, 33))                                        # every admitted count
    assert [sc.maxb(B) for B in (1, 8, 9, 16, 17, 20, 21, 32)] == [8, 8, 16, 16, 20, 20, 32, 32]
    assert {B for F, mul, B, k, _ in sc.TABLE if k == "gaussian"} == {8, 18, 32}
    assert {k for *_, k, _ in sc.TABLE} == set(sc.pc.RBF_NAMES) and {e for *_, e in sc.TABLE} == set(sc.pc.CUTOFF_NAMES)
    for F, mul in sc.LAYOUTS:
        got = {B for f, m, B, _, _ in sc.TABLE if (f, m) == (F, mul)}
        assert got == {4, 8, 16, 20, 32, 5, 17, 21, 29}
        assert {sc.maxb(B) for B in got} == {8, 16, 20, 32} and sum((B + 3) & ~3 != B for B in got) == 4
        assert 1 <= F <= 256 and 1 <= sum(mul) <= 256
    # what the list of layouts is for: C = 256, F = 256 with C small, F = 1, l = 2 only, an l boundary inside a wave at full width
    C = {(F, mul): sum(mul) for F, mul in sc.LAYOUTS}
    assert 256 in C.values() and C[(256, (1, 0, 0))] == 1 and (1, (1, 0, 0)) in C and (3, (0, 0, 256)) in C
    assert sum((86, 85, 85)) == 256 and 86 % 64 != 0 and (86 + 85) % 64 != 0
    assert any(F != mul[0] for F, mul in sc.LAYOUTS)
    assert len(set(sc.TABLE)) == len(sc.TABLE) and len({sc.case_id(*r) for r in sc.TABLE}) == len(sc.TABLE)
    assert set(sc.DIFF_COUNTS) == {4, 5, 8, 9, 16, 17, 20, 21, 32} and all(F + 2 * sum(mul) > 512 for F, mul in sc.DIFF_LAYOUTS)


# ----------------------------------------------------------------------------------------------------------------- edge lists
@pytest.mark.parametrize("kind", sc.LIST_KINDS)
def test_every_list_kind_has_the_degrees_it_claims(kind):
    el = sc.edge_list(kind)
    n = el.n_nodes
    assert n == 215 <= sc.FEW_ROW_NODES and (el.n_edges == 1941 or kind == "symmetric")
    walked = {"directed": [el.c_rowptr], "transpose": [el.n_rowptr], "shuffled": [el.c_rowptr], "symmetric": [el.c_rowptr, el.n_rowptr]}[kind]
    for rowptr in walked:
        seg = np.diff(rowptr)
        assert rowptr.dtype == np.int32 and rowptr[0] == 0 and rowptr[-1] == el.n_edges
        assert seg[sc.BIG_FIRST:sc.POOL_FIRST].tolist() == [63, 64, 65, 127, 128, 129]      # both sides of one and of two groups of 64
        assert seg[64:68].tolist() == [2, 3, 4, 5] and {15, 16, 17, 32, 33} <= set(seg.tolist())   # the list it extends
        assert seg[-1] == 0 and all(seg[k] == 0 for k in sc.ISOLATED)
    assert (el.c_perm is None) == (kind in ("directed", "symmetric")) and el.n_perm is not None
    ei = el.edge_index
    assert len(set((ei[0] * n + ei[1]).tolist())) == el.n_edges and np.all(ei[0] != ei[1])
    for key, rowptr, perm in ((ei[0], el.c_rowptr, el.c_perm), (ei[1], el.n_rowptr, el.n_perm)):
        order = np.arange(el.n_edges) if perm is None else perm
        assert sorted(order.tolist()) == list(range(el.n_edges))
        for i in range(n):
            assert np.all(key[order[rowptr[i]:rowptr[i + 1]]] == i)
    if kind == "directed":            # the 69-node list is its head, edge for edge
        base = wc.edge_list("directed").edge_index
        assert np.array_equal(ei[:, :base.shape[1]], base) and ei[0, base.shape[1]:].min() == sc.BIG_FIRST
        big = ei[:, base.shape[1]:]
        assert set(big[1].tolist()) <= {sc.SKIN_NODE} | set(range(sc.POOL_FIRST, sc.POOL_FIRST + sc.POOL_NODES))
    el2 = sc.edge_list(kind, extra_isolated=513 - n)
    assert el2.n_nodes == 513 and np.array_equal(el2.edge_index, ei) and np.all(np.diff(el2.c_rowptr)[n:] == 0) and np.all(np.diff(el2.n_rowptr)[n:] == 0)


def test_edge_vectors_cutoff_skin_and_mirror():
    for kind in sc.LIST_KINDS:
        el = sc.edge_list(kind)
        vec, beyond = sc.edge_vectors(el)
        ei, d = el.edge_index, vec.norm(dim=1).numpy()
        assert torch.equal(vec, vec.float().double())
        at = (ei[0] == sc.CUTOFF_NODE) | (ei[1] == sc.CUTOFF_NODE)
        skin = ((ei[0] == sc.SKIN_NODE) | (ei[1] == sc.SKIN_NODE)) & ~at
        assert at.sum() >= 1 and np.all(d[at] == sc.CUTOFF) and skin.sum() >= 7 and np.all(d[skin] > sc.CUTOFF)
        live = ~(at | skin)
        assert np.array_equal(beyond.numpy(), ~live) and d[live].min() > 0.69 and d[live].max() < sc.CUTOFF
        d32 = np.linalg.norm(vec.numpy().astype(np.float32), axis=1)                         # in f32 arithmetic too
        assert d32.dtype == np.float32 and np.all(d32[live] < np.float32(sc.CUTOFF)) and np.all(d32[at] == np.float32(sc.CUTOFF)) and np.all(d32[skin] > np.float32(sc.CUTOFF))
        # every long segment holds one dead edge, and the second group of the longest one holds live ones
        walk = (ei[0], el.c_rowptr, el.c_perm) if kind != "transpose" else (ei[1], el.n_rowptr, el.n_perm)
        for k in range(sc.BIG_FIRST, sc.POOL_FIRST):
            order = np.arange(el.n_edges) if walk[2] is None else walk[2]
            seg = order[walk[1][k]:walk[1][k + 1]]
            assert (~live[seg]).sum() == 1 and (len(seg) <= 64 or live[seg[64:]].sum() >= len(seg) - 65)
    el = sc.edge_list("symmetric")
    vec, _ = sc.edge_vectors(el)
    rev = el.n_perm
    assert np.array_equal(rev[rev], np.arange(el.n_edges)) and torch.equal(vec[torch.tensor(rev).long()], -vec)   # an involution, mirrored vectors
    assert np.array_equal(el.edge_index[:, rev], el.edge_index[::-1])


@pytest.mark.parametrize("n", sc.WALK_NODES)
def test_walk_lists(n):
    el = sc.walk_list(n)
    seg = np.diff(el.c_rowptr)
    assert el.n_nodes == n and seg.tolist() == [i % 4 for i in range(n)] and el.c_perm is None
    assert el.n_edges == sum(i % 4 for i in range(n)) and np.diff(el.n_rowptr).sum() == el.n_edges
    if n >= 16:
        assert (np.diff(el.n_rowptr) == 0).sum() >= n // 4 - 3          # nodes nobody lists
    vec, beyond = sc.edge_vectors(el)
    assert vec.shape == (el.n_edges, 3) and int(beyond.sum()) == len(range(5, el.n_edges, 11))


def test_walk_sizes_reach_every_form_of_the_persistent_walk():
    """sb_check: chunk = 32 from 32 768 nodes, else max(1, n / 1024); the grid is min(n, 2 048) workgroups; labels from 8 workgroups on"""
    chunk = lambda n: 32 if n >= 32768 else max(1, n // 1024)
    grid = lambda n: min(n, 2048)
    ns = sc.WALK_NODES
    assert {n for n in ns if grid(n) < 8} == {1, 2, 7} and {n for n in ns if grid(n) >= 8 and grid(n) % 8} == {9, 15, 2047}
    assert min(n for n in ns if n > grid(n)) == 2049                                       # the first looping grid
    assert {chunk(n) for n in ns} == {1, 2, 3, 4, 32}
    assert all(n % chunk(n) for n in (2049, 3071, 3073, 32773)) and 5000 % chunk(5000) == 0   # ragged last chunks, and a whole one
    assert {chunk(2047), chunk(2048)} == {1, 2}


# -------------------------------------------------------------------------------------------------------- the reference itself
def test_reference_is_the_arithmetic_of_the_parity_test():
    """tests/test_gpu_parity.py::_message_case's oracle lines on a case with node_dim != mul[0] and a Gaussian basis"""
    c = sc.message_case(12, (8, 4, 2), 17, "gaussian", "polynomial")
    irreps, ei = "8x0e+4x1o+2x2e", torch.tensor(c.edges.edge_index)
    hr, xr, vr, sr, xir = (t.clone().requires_grad_() for t in (c.h, c.xhat, c.vec, c.s, c.x))
    dist = torch.linalg.norm(vr, dim=-1, keepdim=True)
    rbf = orc.gaussian_rbf(dist, c.p0, c.p1)
    fcut = orc.polynomial_cutoff(dist, c.cutoff)
    rsh = orc.spherical_harmonics(irreps, vr[:, [1, 2, 0]])
    filt = torch.nn.functional.linear(rbf, c.W, c.b) * fcut
    fo = hr.index_select(0, ei[1]) * filt
    g_state, g_edge, m_s = torch.split(fo, [c.C, c.C, 12], dim=-1)
    m_x = orc.elementwise_tp(irreps, xr.index_select(0, ei[1]), g_state) + orc.elementwise_tp(irreps, rsh, g_edge)
    s_ref, x_ref = sr.index_add(0, ei[0], m_s), xir.index_add(0, ei[0], m_x)
    ((s_ref * c.g_s).sum() + (x_ref * c.g_x).sum()).backward()
    for k, want in zip(sc.OUTPUTS, (s_ref, x_ref, hr.grad, xr.grad, vr.grad, sr.grad, xir.grad)):
        assert float((c.ref[k] - want.detach()).abs().max()) <= 1e-13 * max(1.0, float(want.detach().abs().max())), k


def test_forward_reference_edge_by_edge():
    """The forward once more as a loop over edges and channels, from the definition (nn/xpainn.py:140-159) -- and its forms without the
    l = 0 harmonic and without the residual"""
    c = sc.walk_case(9)
    F, C, (m0, m1, m2) = c.F, c.C, c.mul
    for y00, residual in ((None, True), (0.0, True), (0.0, False)):
        s, x = (c.s.clone(), c.x.clone()) if residual else (torch.zeros_like(c.s), torch.zeros_like(c.x))
        for e in range(c.edges.n_edges):
            i, j = int(c.edges.edge_index[0, e]), int(c.edges.edge_index[1, e])
            d = float(c.vec[e].norm())
            if d >= c.cutoff:
                continue
            ux, uy, uz = (c.vec[e] / d).tolist()
            rho = torch.tensor([math.sin(float(f) * d) / (d + 1e-5) for f in c.p0[0]], dtype=torch.float64) * math.sqrt(2.0 / c.cutoff)
            fc = 0.5 * (math.cos(math.pi * d / c.cutoff) + 1.0)
            filt = (c.W @ rho + c.b) * fc
            ex, ey, ez = uy, uz, ux                       # e3nn's axis order
            s3, s5, s15 = math.sqrt(3.0), math.sqrt(5.0), math.sqrt(15.0)
            Y = [[1.0 if y00 is None else y00], [s3 * ex, s3 * ey, s3 * ez],
                 [s15 * ex * ez, s15 * ex * ey, s5 * (ey * ey - 0.5 * (ex * ex + ez * ez)), s15 * ey * ez, 0.5 * s15 * (ez * ez - ex * ex)]]
            g = c.h[j] * filt
            s[i] += g[2 * C:]
            ch = off = 0
            for l, m in enumerate((m0, m1, m2)):
                for u in range(m):
                    for q in range(2 * l + 1):
                        x[i, off + u * (2 * l + 1) + q] += c.xhat[j, off + u * (2 * l + 1) + q] * g[ch + u] + Y[l][q] * g[C + ch + u]
                ch, off = ch + m, off + m * (2 * l + 1)
        got = sc.message_eval(c, torch.float64, y00=y00, residual=residual)
        assert float((got["s_out"] - s).abs().max()) <= 1e-12 and float((got["x_out"] - x).abs().max()) <= 1e-12, (y00, residual)


def test_list_order_does_not_move_the_reference():
    a, b = sc.message_case(*sc.MAIN, 20), sc.message_case(*sc.MAIN, 20, list_kind="shuffled")
    perm = np.random.default_rng(22).permutation(a.edges.n_edges)
    assert np.array_equal(a.edges.edge_index[:, perm], b.edges.edge_index)
    for k in sc.OUTPUTS:
        want = a.ref[k][torch.tensor(perm)] if k == "grad_vec" else a.ref[k]
        assert float((b.ref[k] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), k


def test_diff_reference_is_the_plain_message_on_real_records():
    """``diff_message_ref`` on records formed from the geometry (ops.training_records' layout) is ``message_ref`` without the residual"""
    c = sc.message_case(7, (5, 0, 3), 5)
    rbf, fcut, _ = sc.pc.radial_ref(c.vec, c.rbf_kind, c.cutoff_kind, c.params, c.cutoff)
    ys = orc._sh_e3nn(2, *torch.nn.functional.normalize(c.vec[:, [1, 2, 0]], dim=-1).unbind(-1))
    E, bp = c.edges.n_edges, 8
    rec = torch.cat([rbf * fcut, torch.zeros(E, bp - 5, dtype=torch.float64), fcut, ys[1], ys[2], torch.zeros(E, 3, dtype=torch.float64)], dim=1)
    ds, dx = sc.diff_message_ref(c.h, c.xhat, rec, c.W, c.b, torch.tensor(c.edges.edge_index), 5, 7, c.mul)
    want = sc.message_eval(c, torch.float64, residual=False)
    assert float((ds - want["s_out"]).abs().max()) <= 1e-12 * float(want["s_out"].abs().max())
    assert float((dx - want["x_out"]).abs().max()) <= 1e-12 * float(want["x_out"].abs().max())


# ------------------------------------------------------------------------------------------- the bound has a factor in hand
@pytest.mark.parametrize("row", sc.TABLE, ids=[sc.case_id(*r) for r in sc.TABLE])
def test_f32_restatement_within_half_the_bound(row):
    c = sc.message_case(*row)
    worst = _err32_over_plain(c, sc.OUTPUTS, sc.TOL_F32)
    print(c.id, {k: f"{v:.3f}" for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst
    assert float(c.ref["grad_vec"][c.beyond].abs().max()) == 0.0 and float(c.ref32["grad_vec"][c.beyond].abs().max()) == 0.0


@pytest.mark.parametrize("B", sc.KIND_COUNTS)
@pytest.mark.parametrize("list_kind", sc.LIST_KINDS[1:])
def test_f32_restatement_within_half_the_bound_other_lists(list_kind, B):
    worst = _err32_over_plain(sc.message_case(*sc.MAIN, B, list_kind=list_kind), sc.OUTPUTS, sc.TOL_F32)
    assert max(worst.values()) <= 0.5, worst


@pytest.mark.parametrize("n", sc.WALK_NODES + (512, 513))
def test_f32_restatement_within_half_the_bound_walk_and_few_row_limit(n):
    c = sc.walk_case(n) if n in sc.WALK_NODES else sc.message_case(*sc.MAIN, 20, extra_isolated=n - sc.N_NODES)
    worst = _err32_over_plain(c, sc.OUTPUTS, sc.TOL_F32)
    assert not worst or max(worst.values()) <= 0.5, worst


@pytest.mark.parametrize("B", sc.DIFF_COUNTS)
@pytest.mark.parametrize("layout", sc.DIFF_LAYOUTS, ids=["main", "256"])
def test_f32_restatement_of_the_second_order_triple(layout, B):
    """values, first-order and second-order gradients: the widening takes no effect for any of the ten tensors"""
    c = sc.diff_case(*layout, B)
    worst = _err32_over_plain(c, sc.DIFF_NAMES, sc.TOL_F32)
    print(c.id, {k: f"{v:.3f}" for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst


# ------------------------------------------------------------------------------------------------------------------- power
def _moved(c, bad, names):
    return {k: float((bad[k] - c.ref[k]).abs().max()) / wc.bound(c.ref[k], c.ref32[k], sc.TOL_F32) for k in names}


@pytest.mark.parametrize("B", [1, 4, 5, 8, 9, 16, 17, 20, 21, 32])
def test_power_a_changed_filter(B):
    """the last basis function's column dropped: every output that depends on the filter moves by at least POWER x its bound"""
    c = sc.message_case(*sc.MAIN, B)
    W = c.W.clone()
    W[:, B - 1] = 0.0
    moved = _moved(c, sc.message_eval(c, torch.float64, W=W), ("s_out", "x_out", "grad_h", "grad_xhat", "grad_vec"))
    assert all(v >= POWER for v in moved.values()), moved


@pytest.mark.parametrize("kind", ["directed", "transpose"])
def test_power_a_dropped_group_of_64(kind):
    """The second group of 64 of the 129-edge segment left out of the walk (forward: the center's rows; reverse: the neighbour's) moves
    the walked node's results, and the dL/dvec of those edges is itself far above the bound (an unwritten or zero row would show)."""
    c = sc.message_case(*sc.MAIN, 20, list_kind=kind)
    el = c.edges
    rowptr, perm = (el.c_rowptr, el.c_perm) if kind == "directed" else (el.n_rowptr, el.n_perm)
    k = sc.POOL_FIRST - 1
    order = np.arange(el.n_edges) if perm is None else perm
    seg = order[rowptr[k]:rowptr[k + 1]]
    assert len(seg) == 129
    keep = np.ones(el.n_edges, dtype=bool)
    keep[seg[64:128]] = False
    bad = sc.message_eval(c, torch.float64, edge_index=el.edge_index[:, keep], vec=c.vec[torch.tensor(keep)])
    names = ("s_out", "x_out") if kind == "directed" else ("grad_h", "grad_xhat")
    moved = _moved(c, bad, names)
    assert all(v >= POWER for v in moved.values()), moved
    lost = c.ref["grad_vec"][torch.tensor(~keep)]
    live = ~c.beyond[torch.tensor(~keep)]
    assert int(live.sum()) >= 62 and float(lost[live].abs().max()) >= POWER * wc.bound(c.ref["grad_vec"], c.ref32["grad_vec"], sc.TOL_F32)
    # ... and so does the segment's very last edge (the third group, one edge long)
    keep[:] = True
    keep[seg[128]] = False
    bad = sc.message_eval(c, torch.float64, edge_index=el.edge_index[:, keep], vec=c.vec[torch.tensor(keep)])
    assert all(v >= POWER for v in _moved(c, bad, names).values()) or bool(c.beyond[seg[128]])


@pytest.mark.parametrize("n,node", [(9, 7), (2049, 2047), (3073, 3071), (5000, 4999), (32773, 32771)])
def test_power_a_dropped_walk_item(n, node):
    """one node of the ragged tail never visited: its row of s_out / x_out would be the residual alone"""
    c = sc.walk_case(n)
    el = c.edges
    assert node % 4 == 3
    keep = el.edge_index[0] != node
    bad = sc.message_eval(c, torch.float64, edge_index=el.edge_index[:, keep], vec=c.vec[torch.tensor(keep)])
    moved = _moved(c, bad, ("s_out", "x_out"))
    assert all(v >= POWER for v in moved.values()), moved


@pytest.mark.parametrize("B", [4, 17])
def test_power_of_the_second_order_comparison(B):
    c = sc.diff_case(*sc.MAIN, B)
    w = c.w.clone()
    w[:, B - 1] = 0.0
    bad = sc.diff_message_eval(c, torch.float64, w=w)
    moved = {k: float((bad[k] - c.ref[k]).abs().max()) / wc.bound(c.ref[k], c.ref32[k], sc.TOL_F32) for k in sc.DIFF_NAMES}
    assert all(v >= POWER for v in moved.values()), moved
