"""The case builder and references of tests/painn_kernel_cases.py on the host: the references against the existing oracle on the
reference's own molecule, the edge lists against what they claim, and the POWER of the comparison that tests/test_gpu_painn_kernels.py
makes -- the f64 reference evaluated a second time with one deliberate defect must move an output by at least 10 x the bound the GPU
test uses for that output, or that bound could hide a wrong kernel."""
import json
import os

import numpy as np
import pytest
import torch

from tests import painn_kernel_cases as pc, painn_oracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POWER = 10.0


def _rel(a, b):
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def test_references_reproduce_the_oracle_on_the_fixture_molecule():
    """Bessel + cosine, h = scalar_mlp(s): message_ref / update_uv_ref + update_out_ref equal painn_oracle.message / update (which
    tests/test_painn_host.py pins to painn_model_f64.npz) to 1e-12, forward and reverse, on a state with x != 0."""
    from tests.test_painn_host import _reference_buffers

    f = np.load(os.path.join(GOLDEN, "painn_model_f64.npz"))
    shapes = json.load(open(os.path.join(GOLDEN, "painn_keys.json")))["gfn2-xtb"]
    p = _reference_buffers(po.seeded_weights(shapes, int(f["seed"])))
    pos, ei = torch.tensor(f["mol_pos"]), torch.tensor(f["mol_edge_index"])
    vec0 = po.edge_vectors(pos, ei)
    s, x = po.embedding(torch.tensor(f["mol_z"]).long(), p), None
    x = torch.zeros((s.shape[0], 3, s.shape[1]), dtype=s.dtype)
    s, x = po.message(s, x, *po.radial(vec0, p["embedding.rbf.freq"], 5.0), ei, p, "message_0.")
    s, x = po.update(s, x, p, "update_0.")
    gen = torch.Generator().manual_seed(0)
    g_s, g_x = torch.randn(s.shape, dtype=torch.float64, generator=gen), torch.randn(x.shape, dtype=torch.float64, generator=gen)
    params = (p["embedding.rbf.freq"],)

    def leaves():
        return s.clone().requires_grad_(), x.clone().requires_grad_(), vec0.clone().requires_grad_()

    s1, x1, v1 = leaves()
    want = po.message(s1, x1, *po.radial(v1, p["embedding.rbf.freq"], 5.0), ei, p, "message_1.")
    want_g = torch.autograd.grad(want, [s1, x1, v1], [g_s, g_x])
    s2, x2, v2 = leaves()
    h = po._mlp(s2, p, "message_1.scalar_mlp")
    got = pc.message_ref(s2, x2, h, v2, ei, p["message_1.rbf_lin.weight"], p["message_1.rbf_lin.bias"], "bessel", "cosine", params, 5.0)
    got_g = torch.autograd.grad(got, [s2, x2, v2], [g_s, g_x])
    for a, b in zip(list(got) + list(got_g), list(want) + list(want_g)):
        assert _rel(a.detach(), b.detach()) <= 1e-12

    s1, x1, _ = leaves()
    want = po.update(s1, x1, p, "update_1.")
    want_g = torch.autograd.grad(want, [s1, x1], [g_s, g_x])
    s2, x2, _ = leaves()
    U, V, ip, cat = pc.update_uv_ref(s2, x2, p["update_1.update_U.weight"], p["update_1.update_V.weight"])
    a = po._mlp(cat, p, "update_1.update_mlp")
    got = pc.update_out_ref(s2, x2, a, U, ip)
    got_g = torch.autograd.grad(got, [s2, x2], [g_s, g_x])
    for a_, b_ in zip(list(got) + list(got_g), list(want) + list(want_g)):
        assert _rel(a_.detach(), b_.detach()) <= 1e-12
    assert float(x[-1].abs().max()) == 0.0 and torch.isfinite(got_g[1]).all()   # the single atom: V = 0, a zero subgradient


@pytest.mark.parametrize("rbf_kind", pc.RBF_NAMES)
@pytest.mark.parametrize("cutoff_kind", pc.CUTOFF_NAMES)
def test_radial_reference_is_what_the_projects_modules_describe(rbf_kind, cutoff_kind):
    """p0 / p1 handed to the kernel and the parameters handed to the reference are the same numbers; the envelope is zero from the
    cutoff on and one at d = 0."""
    sp = pc.radial_spec(rbf_kind, cutoff_kind, 8, 3.7)
    assert sp["p0"].shape == (1, 8) and sp["p0"].dtype == torch.float32 and (sp["p1"] is None) == (rbf_kind == "bessel")
    vec = torch.tensor([[1e-9, 0.0, 0.0], [0.0, 1.3, 0.0], [0.0, 0.0, float(np.float32(3.7))], [4.0, 0.0, 0.0]], dtype=torch.float64)
    rbf, fcut, u = pc.radial_ref(vec, rbf_kind, cutoff_kind, sp["rbf_params"], sp["cutoff"])
    assert rbf.shape == (4, 8) and torch.isfinite(rbf[1:]).all()
    assert abs(float(fcut[0]) - 1.0) < 1e-12 and 0.0 < float(fcut[1]) < 1.0 and float(fcut[2]) == 0.0 and float(fcut[3]) == 0.0
    first = {"bessel": sp["rbf_params"][0], "gaussian": sp["rbf_params"][0], "expnorm": sp["rbf_params"][0]}.get(rbf_kind)
    if first is not None:
        assert torch.equal(first.reshape(-1), sp["p0"].reshape(-1))
    else:   # expbern: p0 = softplus(_alpha) once per basis function, p1 = the log binomials
        assert torch.allclose(sp["p0"], torch.nn.functional.softplus(sp["rbf_params"][0]).expand(1, 8)) and torch.equal(sp["p1"].reshape(-1), sp["rbf_params"][1])


def _segments(rowptr):
    return np.diff(rowptr)


@pytest.mark.parametrize("kind", pc.LIST_KINDS)
def test_every_list_kind_has_the_degrees_it_claims(kind):
    el = pc.edge_list(kind)
    n = el.n_nodes
    walked = {"directed": [el.c_rowptr], "transpose": [el.n_rowptr], "shuffled": [el.c_rowptr], "symmetric": [el.c_rowptr, el.n_rowptr]}[kind]
    for rowptr in walked:
        seg = _segments(rowptr)
        assert rowptr.dtype == np.int32 and rowptr[0] == 0 and rowptr[-1] == el.n_edges
        assert set(pc.CLAIMED) <= set(seg.tolist()), sorted(set(seg.tolist()))
        assert seg[-1] == 0 and any(seg[k] == 0 for k in range(1, n - 1))   # the last node and an interior one
    assert (el.c_perm is None) == (kind in ("directed", "symmetric")) and el.n_perm is not None
    assert len(set((el.edge_index[0] * n + el.edge_index[1]).tolist())) == el.n_edges and np.all(el.edge_index[0] != el.edge_index[1])
    # the views are what they say: walking a row through perm meets exactly the edges of that row, in list order
    for key, rowptr, perm in ((el.edge_index[0], el.c_rowptr, el.c_perm), (el.edge_index[1], el.n_rowptr, el.n_perm)):
        order = np.arange(el.n_edges) if perm is None else perm
        assert perm is None or perm.dtype == np.int32
        assert sorted(order.tolist()) == list(range(el.n_edges))
        for i in range(n):
            assert np.all(key[order[rowptr[i]:rowptr[i + 1]]] == i)
    if kind == "directed":   # nodes nobody lists: the reverse walk has empty rows with g_x_in = g_x
        assert all(_segments(el.n_rowptr)[j] == 0 for j in pc.ISOLATED + pc.SOURCES)


def test_the_reverse_edge_map_is_an_involution_that_sorts_by_neighbour():
    el = pc.edge_list("symmetric")
    rev, ei = el.n_perm, el.edge_index
    assert np.array_equal(rev[rev], np.arange(el.n_edges))
    assert np.array_equal(ei[0][rev], ei[1]) and np.array_equal(ei[1][rev], ei[0])
    assert np.array_equal(rev, np.argsort(ei[1], kind="stable"))   # the permutation the stable sort by neighbour gives
    base = pc.edge_list("directed").edge_index
    both = set(map(tuple, base.T.tolist())) | set(map(tuple, base[::-1].T.tolist()))
    assert both == set(map(tuple, ei.T.tolist()))


def test_edge_vectors_have_the_skin_and_the_cutoff_edges():
    for kind in pc.LIST_KINDS:
        for cutoff in (5.0, 3.7):
            c = pc.message_case(64, 8, cutoff=cutoff, list_kind=kind)
            d32 = np.linalg.norm(c.vec.numpy().astype(np.float32), axis=1)
            d = c.vec.norm(dim=1).numpy()
            at = d32 == np.float32(cutoff)
            assert at.sum() >= 1 and np.all(d[at] == float(np.float32(cutoff)))
            skin = (d > cutoff) & ~at
            assert skin.sum() >= 6 and np.all(d[skin] < 1.2001 * cutoff) and np.all(d[~skin & ~at] < 0.9501 * cutoff) and d.min() > 0.29
            assert np.array_equal(c.beyond.numpy(), at | skin)
            assert torch.equal(c.vec, c.vec.float().double())


# ------------------------------------------------------------------------------------------------------------------- power
def _moved(ref, bad, ref32, names):
    """min over ``names`` of |defective - correct| / bound"""
    return {k: float((bad[k] - ref[k]).abs().max()) / pc.bound(ref[k], ref32[k]) for k in names}


def _assert_power(ref, bad, ref32, names, what):
    moved = _moved(ref, bad, ref32, names)
    assert all(v >= POWER for v in moved.values()), (what, moved)


def _neighbour_block(t, F):
    """the last 16 channels of every F-wide slice taken from the 16 in front of them"""
    out = t.clone().reshape(-1, F)
    out[:, F - 16:] = out[:, F - 32:F - 16]
    return out.reshape(t.shape)


def _row_left(t, fill=0.0):
    out = t.clone()
    out[-1] = fill
    return out


@pytest.mark.parametrize("F, list_kind", [(32, "directed"), (256, "directed"), (128, "symmetric"), (96, "transpose")])
def test_power_of_the_message_comparison(F, list_kind):
    c = pc.message_case(F, 20, list_kind=list_kind)
    el, ref, ref32 = c.edges, c.ref, c.ref32
    ei = torch.tensor(el.edge_index)
    both, fwd, rev = pc.MESSAGE_OUTPUTS, ("s_out", "x_out"), ("g_h", "g_x_in", "g_vec")

    # the last edge of a 17-edge segment dropped: from the forward walk, and from the reverse walk
    walks = 0
    for rowptr, perm, names in ((el.c_rowptr, el.c_perm, fwd), (el.n_rowptr, el.n_perm, ("g_h", "g_x_in"))):
        seg = np.diff(rowptr)
        if 17 not in seg:   # (the walk of this list kind that does not carry the claimed degrees)
            continue
        walks += 1
        row = int(np.nonzero(seg == 17)[0][0])
        slot = int(rowptr[row + 1]) - 1
        e = slot if perm is None else int(perm[slot])
        assert not bool(c.beyond[e])
        keep = torch.arange(el.n_edges) != e
        bad = pc.message_eval(c, torch.float64, edge_index=ei[:, keep], vec=c.vec[keep])
        _assert_power(ref, bad, ref32, names, "edge 17 of a segment dropped")
    assert walks >= 1
    g_vec_lost = ref["g_vec"][e].abs().max() / pc.bound(ref["g_vec"], ref32["g_vec"])   # dL/dvec of that edge left at zero
    assert float(g_vec_lost) >= POWER, float(g_vec_lost)

    w = c.w.clone()
    w[:, -1] = 0.0
    _assert_power(ref, pc.message_eval(c, torch.float64, w=w), ref32, both, "last basis function dropped")
    _assert_power(ref, pc.message_eval(c, torch.float64, b=torch.zeros_like(c.b)), ref32, both, "bias column dropped")
    shifted = {k: _neighbour_block(ref[k], F) for k in ("s_out", "x_out", "g_h", "g_x_in")}
    _assert_power(ref, shifted, ref32, tuple(shifted), "last 16 channels from the neighbouring block")
    _assert_power(ref, pc.message_eval(c, torch.float64, keep_envelope_gradient=False), ref32, ("g_vec",), "envelope derivative dropped")
    # node row n - 1 left unwritten (at zero).  The last node is isolated: s_out = s, x_out = x, g_x_in = g_x there; g_h is exactly
    # zero on it, which no value can tell from a row left at zero -- the GPU test's never-written pattern does
    left = {k: _row_left(ref[k]) for k in ("s_out", "x_out", "g_x_in")}
    _assert_power(ref, left, ref32, tuple(left), "row n - 1 left unwritten")


@pytest.mark.parametrize("rbf_kind", pc.RBF_NAMES)
@pytest.mark.parametrize("cutoff_kind", pc.CUTOFF_NAMES)
def test_power_of_the_radial_and_envelope_sweep(rbf_kind, cutoff_kind):
    """Every radial kind and envelope of the GPU sweep (F = 64, B = 8): a dropped last basis function, a dropped bias column and a
    dropped envelope derivative are each seen."""
    c = pc.message_case(64, 8, rbf_kind, cutoff_kind)
    w = c.w.clone()
    w[:, -1] = 0.0
    _assert_power(c.ref, pc.message_eval(c, torch.float64, w=w), c.ref32, pc.MESSAGE_OUTPUTS, "last basis function dropped")
    _assert_power(c.ref, pc.message_eval(c, torch.float64, b=torch.zeros_like(c.b)), c.ref32, pc.MESSAGE_OUTPUTS, "bias column dropped")
    _assert_power(c.ref, pc.message_eval(c, torch.float64, keep_envelope_gradient=False), c.ref32, ("g_vec",), "envelope derivative dropped")
    other = pc.message_case(64, 8, rbf_kind, "polynomial" if cutoff_kind == "cosine" else "cosine")
    swapped = pc.message_eval(SimpleSpec(c, other.spec), torch.float64)
    _assert_power(c.ref, swapped, c.ref32, pc.MESSAGE_OUTPUTS, "the other envelope")


class SimpleSpec:
    """a case with another radial spec"""

    def __init__(self, case, spec):
        self.__dict__.update(case.__dict__)
        self.spec = spec


@pytest.mark.parametrize("F, n", [(32, 33), (256, 17), (96, 2049)])
def test_power_of_the_update_comparison(F, n):
    c = pc.update_case(F, n)
    ref, ref32 = c.ref, c.ref32
    _assert_power(ref, pc.update_eval(c, torch.float64, swap_uv=True), ref32, ("U", "V", "cat", "x_out", "g_a", "g_x_in"), "U and V swapped")
    a = torch.cat([c.a[:, :F], c.a[:, 2 * F:], c.a[:, F:2 * F]], dim=1)
    _assert_power(ref, pc.update_eval(c, torch.float64, a=a), ref32, ("s_out", "x_out", "g_x_in"), "a_vv / a_sv swapped")
    g_a = ref["g_a"]   # the same swap on the way back
    bad = {"g_a": torch.cat([g_a[:, :F], g_a[:, 2 * F:], g_a[:, F:2 * F]], dim=1)}
    _assert_power(ref, bad, ref32, ("g_a",), "a_vv / a_sv swapped in dL/da")
    shifted = {k: _neighbour_block(ref[k], F) for k in pc.UPDATE_OUTPUTS}
    _assert_power(ref, shifted, ref32, pc.UPDATE_OUTPUTS, "last 16 channels from the neighbouring block")
    # row n - 1 left unwritten (at zero).  It is a row with x = 0: U, V, <U, V>, x_out and the a_vv part of dL/da are exactly zero
    # there, which no value can tell from a row left at zero -- the GPU test's never-written pattern does
    assert c.zero_rows[-1] == n - 1 and float(ref["V"][-1].abs().max()) == 0.0
    left = {k: _row_left(ref[k]) for k in ("cat", "s_out", "g_a", "g_s_in", "g_x_in")}
    _assert_power(ref, left, ref32, tuple(left), "row n - 1 left unwritten")
    full = pc.update_case(F, n, zero_rows=False)
    left = {k: _row_left(full.ref[k]) for k in pc.UPDATE_OUTPUTS}
    _assert_power(full.ref, left, full.ref32, pc.UPDATE_OUTPUTS, "row n - 1 left unwritten (x != 0)")


def test_zero_rows_have_a_zero_norm_and_a_finite_reverse():
    c = pc.update_case(32, 17)
    assert c.zero_rows == (pc.ZERO_ROW_INSIDE, 16)
    for r in c.zero_rows:
        assert float(c.ref["V"][r].abs().max()) == 0.0 and float(c.ref["cat"][r, 32:].abs().max()) == 0.0
        assert torch.isfinite(c.ref["g_x_in"][r]).all() and torch.isfinite(c.ref32["g_x_in"][r]).all()   # |V| = 0: a zero subgradient, not 0 / 0


def test_packed_filter_layout():
    w, b = torch.arange(6.0).reshape(3, 2), torch.tensor([10.0, 11.0, 12.0])
    out = pc.packed_filter(w, b)
    assert out.shape == (pc.KPAD, 3) and torch.equal(out[:2], w.T) and torch.equal(out[2], b) and float(out[3:].abs().max()) == 0.0
