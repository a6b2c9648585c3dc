"""Table form of the first message block (include/xeq.h: xeq_message_fwd_wq_table / _bwd_wq_table): h and the 0e block of xhat read from
the element table's rows instead of from the per-node copies that xeq_first_block_front gathers.

Every comparison is ``torch.equal`` / ``np.array_equal`` against the existing first-block form (XEQ_XHAT_HIGHER_L_ZERO, no node gradients)
fed with the gathered copies of the same table: the values read are the same floats and every sum keeps its order, so no tolerance
applies.  Shapes: three molecules of 5 / 9 / 23 atoms, repeated so that a launch has more than one workgroup per unit, four species and
one table row no atom uses, out-degrees that include 1, 4, 5 (a quad boundary) and 17 (a tile boundary), one atom without an edge."""
import numpy as np
import pytest
import torch

from tests import wq_message_cases as wc
from xequinet_amd import lib

DEV = "cuda"
MUL = wc.MUL_MAIN
B = 20
SIZES = (5, 9, 23)
REPEATS = 4
DEGREES = (1, 4, 5, 17, 3, 8, 2)
T_ROWS = 5          # rows 1 .. 4 are species, row 0 is used by no atom


def _edges(wide):
    """Directed list, centers ascending.  ``wide``: a center's neighbours are spread over ALL atoms (a step's gradient window then spans
    every node and does not fit LDS); else they are the next atoms of its own molecule.  The last atom of every 5-atom molecule has no
    edge in either direction."""
    sizes = SIZES * REPEATS
    n = sum(sizes)
    src, dst, first = [], [], 0
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    lone = [int(s0) + 4 for s0, size in zip(starts, sizes) if size == 5]
    for size in sizes:
        members = list(range(first, first + size - (1 if size == 5 else 0)))
        for k, i in enumerate(members):
            deg = min(DEGREES[(i + k) % len(DEGREES)], len(members) - 1)
            if wide:
                pool = [j for j in range(n) if j != i and j not in lone]
                stride = max(1, len(pool) // 17)
                nbrs = sorted({pool[(i * 7 + stride * q) % len(pool)] for q in range(deg)})
            else:
                nbrs = sorted(members[(k + 1 + q) % len(members)] for q in range(deg))
            src += [i] * len(nbrs)
            dst += nbrs
        first += size
    ei = np.array([src, dst], dtype=np.int64)
    out_deg = np.bincount(ei[0], minlength=n)
    assert {1, 4, 5, 17} <= set(out_deg.tolist()) or wide
    assert all(out_deg[i] == 0 and not (ei[1] == i).any() for i in lone)
    return ei, n


def _case(wide=False, z_dtype=torch.int32):
    ei, n = _edges(wide)
    F, C, D = MUL[0], sum(MUL), MUL[0] + 3 * MUL[1] + 5 * MUL[2]
    H = F + 2 * C
    g = torch.Generator().manual_seed(7 + int(wide))
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32)
    z = torch.randint(1, T_ROWS, (n,), generator=g)
    assert set(z.tolist()) == {1, 2, 3, 4}
    h_t, x0_t = r(T_ROWS, H), r(T_ROWS, F)
    vec = r(ei.shape[1], 3)
    vec = vec / vec.norm(dim=1, keepdim=True) * (0.8 + 3.5 * torch.rand(ei.shape[1], 1, generator=g))      # inside the cutoff
    p0, p1 = wc.radial_params("bessel", "cosine", B)
    xhat = torch.cat([x0_t[z].reshape(-1), torch.zeros(n * (D - F))])                                       # BT layout: the 0e block first
    d = lambda t: t.to(DEV).contiguous()
    return dict(n=n, ei=d(torch.tensor(ei)), z=d(z.to(z_dtype)), h_t=d(h_t), x0_t=d(x0_t), h=d(h_t[z]), xhat=d(xhat), vec=d(vec), s=d(r(n, F)),
                x=d(r(n, D)), g_s=d(r(n, F)), g_x=d(r(n, D)), W=d(r(H, B) / B ** 0.5), b=d(r(H)), p0=d(p0.float()), p1=None if p1 is None else d(p1.float()))


def _run(c, table, symmetric_graph=None):
    """forward, the reverse launch's per-unit partials, dL/dvec -- through ops.message_forward / message_backward"""
    from xequinet_amd import ops

    graph = ops.EdgeGraph(c["ei"], c["n"]) if symmetric_graph is None else symmetric_graph
    flags = 1 | lib.XHAT_HIGHER_L_ZERO
    cfg = ("bessel", "cosine", B, wc.CUTOFF, MUL[0], MUL, flags) + (((c["z"], c["h_t"], c["x0_t"]),) if table else ())
    n0 = lib.launch_count()
    s_out, x_out, saved, impl = ops.message_forward(c["h"], c["xhat"], c["vec"], c["s"], c["x"], c["W"], c["b"], c["p0"], c["p1"], graph, cfg,
                                                    want_backward=True)
    assert impl == "wq"
    keep = ops.EdgeGradDeferral()      # waits for two blocks: the first one's partials stay with it
    keep.register(), keep.register()
    assert ops.message_backward(saved, graph, cfg, impl, c["g_s"], c["g_x"], node_grads=False, deferral=keep)[2] is None
    g_vec = ops.message_backward(saved, graph, cfg, impl, c["g_s"], c["g_x"], node_grads=False)[2]
    names = lib.launch_names(n0)
    plan = next(p for key, p in graph._wq.items() if key[0] == (not graph.mirror_walk))
    used = 4 * int(plan["qptr"][c["n"]].item())                                   # padded slots of the walk: the rest of a row is never written
    parts = keep.sets[0].view(-1, plan["pcap"])[:, :used]
    torch.cuda.synchronize()
    assert ("xeq_message_fwd_wq_table" in names) == table and ("xeq_message_bwd_wq_table" in names) == table, names
    assert names.count("xeq_edge_basis_wq") == (1 if graph.mirror_walk else 2), names   # the table rows cost no launch
    return {"s_out": s_out, "x_out": x_out, "grad_vec": g_vec, "parts": parts.clone()}


def _same(a, b, what):
    for k in ("s_out", "x_out", "grad_vec", "parts"):
        assert torch.isfinite(a[k]).all(), (what, k)
        assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), (what, k, float((a[k] - b[k]).abs().max()))
    assert float(a["grad_vec"].abs().max()) > 0 and float((a["s_out"] - b["s_out"]).abs().max()) == 0


@pytest.fixture(autouse=True)
def _wq(monkeypatch):
    monkeypatch.setenv("XEQ_MESSAGE_IMPL", "wq")
    monkeypatch.delenv("XEQ_WQ_EDGES_PER_STREAM", raising=False)
    monkeypatch.delenv("XEQ_WQ_LONG_MULT", raising=False)
    monkeypatch.delenv("XEQ_WQ_FIRST_TABLE", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("z_dtype", [torch.int32, torch.int64], ids=["z32", "z64"])
@pytest.mark.parametrize("eps", [None, "48", "80"], ids=["epsdefault", "eps48", "eps80"])
def test_table_form_is_the_first_block_form_bit_for_bit(eps, z_dtype, monkeypatch):
    if eps is not None:
        monkeypatch.setenv("XEQ_WQ_EDGES_PER_STREAM", eps)
    c = _case(z_dtype=z_dtype)
    _same(_run(c, True), _run(c, False), f"eps {eps}")


@pytest.mark.gpu
def test_table_form_on_a_symmetric_list_walks_the_forward_plan():
    """mirror walk: one record launch writes the slots' rows for the forward kernel and the quads' rows for the reverse kernel"""
    from xequinet_amd import ops

    c = _case()
    ei = c["ei"].cpu()
    both = torch.cat([ei, ei.flip(0)], dim=1)
    both = torch.unique(both, dim=1)                                              # sorted by center, then neighbour
    g = torch.Generator().manual_seed(3)
    vec = torch.randn(both.shape[1], 3, generator=g)
    c = dict(c, ei=both.to(DEV).contiguous(), vec=(vec / vec.norm(dim=1, keepdim=True) * 2.0).to(DEV).contiguous())
    graphs = [ops.EdgeGraph(c["ei"], c["n"], center_sorted=True, symmetric=True) for _ in range(2)]
    assert graphs[0].mirror_walk
    _same(_run(c, True, graphs[0]), _run(c, False, graphs[1]), "mirror")


@pytest.mark.gpu
def test_table_form_when_a_steps_gradient_window_does_not_fit():
    """A center's neighbours are spread over all 148 atoms; 148 rows of the widest kind (l = 2: 640 bytes) are more than any window the
    reverse kernel keeps (48 KB at most), so its steps gather the centers' gradients from global memory while the owners' rows still
    come from the table."""
    c = _case(wide=True)
    assert c["n"] * 640 > 48 * 1024
    _same(_run(c, True), _run(c, False), "wide")


@pytest.mark.gpu
def test_a_number_outside_the_table_reads_row_zero():
    c = _case()
    z = c["z"].clone()
    z[3], z[11] = 77, -2
    zc = z.clamp(0, T_ROWS - 1).long()
    zc[3] = zc[11] = 0
    F = MUL[0]
    xhat = c["xhat"].clone()
    xhat[: c["n"] * F] = c["x0_t"][zc].reshape(-1)
    c = dict(c, z=z, h=c["h_t"][zc].contiguous(), xhat=xhat)
    _same(_run(c, True), _run(c, False), "outside")


# ------------------------------------------------------------------------------------------------------------------ whole model
def _eval(model, pos, z, ptr, graphed):
    from xequinet_amd.data import NeighborTransform, XequiBatch
    from xequinet_amd.runtime import GraphedStep, pair_capacity

    t = lambda a, dt=None: torch.tensor(a, dtype=dt).to(DEV)
    n0 = lib.launch_count()
    if graphed:
        step = GraphedStep(model, (len(pos), len(ptr) - 1, pair_capacity(ptr)))
        for _ in range(2):                                                        # the second call is a replay
            out = step(t(pos, torch.float32), t(z), t(ptr), ptr_host=ptr)
        res = out["energy"].clone(), out["forces"].clone()
    else:
        batch = NeighborTransform(model.cutoff_radius)(XequiBatch(t(pos, torch.float32), t(z), t(ptr)))
        with torch.enable_grad():
            out = model(batch.to_dict(), compute_forces=True, compute_virial=False)
        res = out["energy"].detach().clone(), out["forces"].detach().clone()
    torch.cuda.synchronize()
    return res, lib.launch_names(n0)


@pytest.mark.gpu
@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph_replay"])
def test_whole_evaluation_equals_the_run_with_the_table_form_switched_off(graphed, monkeypatch):
    from xequinet_amd.data import synthetic as syn
    from xequinet_amd.nn import resolve_model

    monkeypatch.delenv("XEQ_MESSAGE_IMPL")                                        # 64 QM9-shape molecules: the automatic choice is wq
    torch.manual_seed(0)
    model = resolve_model("xpainn").to(DEV).eval().requires_grad_(False)
    pos, z, ptr = syn.synth_qm9_batch(64, seed=11)
    _eval(model, pos, z, ptr, False)                                              # (the packed-weight caches fill here, not in a compared run)
    (e_on, f_on), names_on = _eval(model, pos, z, ptr, graphed)
    monkeypatch.setenv("XEQ_WQ_FIRST_TABLE", "0")
    (e_off, f_off), names_off = _eval(model, pos, z, ptr, graphed)
    assert "xeq_message_fwd_wq_table" in names_on and "xeq_message_bwd_wq_table" in names_on, names_on
    assert not any(n.endswith("_table") and n.startswith("xeq_message") for n in names_off), names_off
    assert [n.replace("_wq_table", "_wq") for n in names_on] == names_off          # the same launches in the same order
    assert torch.isfinite(f_on).all() and float(f_on.abs().max()) > 0
    assert np.array_equal(e_on.cpu().numpy(), e_off.cpu().numpy()) and np.array_equal(f_on.cpu().numpy(), f_off.cpu().numpy())


@pytest.mark.gpu
def test_a_list_without_the_mirror_walk_keeps_its_two_record_launches(monkeypatch):
    """A plain edge list (no promise of symmetry) walks a reverse plan of its own, whose records the LAST block's reverse pass requests
    first: that launch has to write the table rows the first block's reverse pass reads, or the records would be written twice."""
    from oracle import xpainn_oracle as orc
    from xequinet_amd.data import synthetic as syn
    from xequinet_amd.nn import resolve_model

    monkeypatch.delenv("XEQ_MESSAGE_IMPL")
    torch.manual_seed(0)
    model = resolve_model("xpainn").to(DEV).eval().requires_grad_(False)
    pos, z, ptr = syn.synth_qm9_batch(64, seed=11)
    ei = orc.radius_graph_canonical(pos.astype(np.float32), ptr, model.cutoff_radius)
    t = lambda a, dt=None: torch.tensor(a, dtype=dt).to(DEV)
    res = {}
    for flag in ("1", "1", "0"):                                                  # (the first run fills the pack caches)
        monkeypatch.setenv("XEQ_WQ_FIRST_TABLE", flag)
        data = {"pos": t(pos, torch.float32), "atomic_numbers": t(z), "edge_index": t(ei), "ptr": t(ptr),
                "batch": t(np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)))}
        n0 = lib.launch_count()
        with torch.enable_grad():
            out = model(data, compute_forces=True, compute_virial=False)
        torch.cuda.synchronize()
        res[flag] = (out["energy"].detach().clone(), out["forces"].detach().clone(), lib.launch_names(n0))
    assert "xeq_message_bwd_wq_table" in res["1"][2] and res["1"][2].count("xeq_edge_basis_wq") == 2
    assert [n.replace("_wq_table", "_wq") for n in res["1"][2]] == res["0"][2]
    assert torch.equal(res["1"][0], res["0"][0]) and torch.equal(res["1"][1], res["0"][1])


@pytest.mark.gpu
def test_native_operator_takes_the_table_form_too(monkeypatch):
    from xequinet_amd.data import synthetic as syn
    from xequinet_amd.interface.scripted import XPaiNNNative
    from xequinet_amd.nn import resolve_model
    from oracle import xpainn_oracle as orc

    monkeypatch.delenv("XEQ_MESSAGE_IMPL")
    torch.manual_seed(0)
    model = resolve_model("xpainn").to(DEV).eval().requires_grad_(False)
    pos, z, ptr = syn.synth_qm9_batch(64, seed=11)
    ei = orc.radius_graph_canonical(pos.astype(np.float32), ptr, model.cutoff_radius)
    t = lambda a, dt=None: torch.tensor(a, dtype=dt).to(DEV)
    native = XPaiNNNative(model)
    native(t(pos, torch.float32), t(z.astype(np.int32)), t(ei), t(ptr), None, None, True, True, True, False)    # (fills the pack caches)
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("XEQ_WQ_FIRST_TABLE", flag)
        n0 = lib.launch_count()
        out = native(t(pos, torch.float32), t(z.astype(np.int32)), t(ei), t(ptr), None, None, True, True, True, False)
        torch.cuda.synchronize()
        res[flag] = (out[0].clone(), out[2].clone(), lib.launch_names(n0))
    assert "xeq_message_fwd_wq_table" in res["1"][2] and "xeq_message_bwd_wq_table" in res["1"][2]
    assert [n.replace("_wq_table", "_wq") for n in res["1"][2]] == res["0"][2]
    assert torch.equal(res["1"][0], res["0"][0]) and torch.equal(res["1"][1], res["0"][1])


@pytest.mark.gpu
def test_a_charged_model_keeps_its_launches(monkeypatch):
    """behind a charge embedding the first block's front half runs per node: no table form, the launch names of the form switched off"""
    from xequinet_amd.data import NeighborTransform, XequiBatch
    from xequinet_amd.data import synthetic as syn
    from xequinet_amd.nn import resolve_model

    monkeypatch.delenv("XEQ_MESSAGE_IMPL")
    torch.manual_seed(0)
    model = resolve_model("xpainn", charge_embed=True).to(DEV).eval().requires_grad_(False)
    pos, z, ptr = syn.synth_qm9_batch(64, seed=11)
    t = lambda a, dt=None: torch.tensor(a, dtype=dt).to(DEV)
    seqs = {}
    for flag in ("1", "1", "0"):                                                  # (the first run fills the pack caches)
        monkeypatch.setenv("XEQ_WQ_FIRST_TABLE", flag)
        batch = NeighborTransform(model.cutoff_radius)(XequiBatch(t(pos, torch.float32), t(z), t(ptr), charge=torch.ones(len(ptr) - 1)).to(DEV))
        data = batch.to_dict()
        n0 = lib.launch_count()
        with torch.enable_grad():
            out = model(data, compute_forces=True, compute_virial=False)
        torch.cuda.synchronize()
        seqs[flag] = lib.launch_names(n0)
        assert torch.isfinite(out["forces"]).all()
    assert seqs["1"] == seqs["0"] and not any(n.endswith("_wq_table") for n in seqs["1"]), seqs["1"]
    assert any(n.startswith("xeq_message_fwd_wq") for n in seqs["1"]) and "xeq_electronic_mix" in seqs["1"], seqs["1"]


# --------------------------------------------------------------------------------------------------------- selection (host only)
def test_selection_keeps_the_old_form_where_the_table_form_does_not_apply(monkeypatch):
    monkeypatch.delenv("XEQ_WQ_FIRST_TABLE", raising=False)
    L = lib.load()
    WQ, SB, GENERIC = 0, 1, 3                                                     # XEQ_FAMILY_* of include/xeq.h
    rows_max = int(L.xeq_message_wq_table_max_rows())
    assert 87 <= rows_max <= 128                                                  # the model's element table has 87 rows
    assert L.xeq_message_wq_first_table(WQ, 87, 0, 0) == 1 and L.xeq_message_wq_first_table(WQ, 1, 0, 0) == 1
    assert L.xeq_message_wq_first_table(WQ, rows_max, 0, 0) == 1 and L.xeq_message_wq_first_table(WQ, rows_max + 1, 0, 0) == 0
    assert L.xeq_message_wq_first_table(WQ, 129, 0, 0) == 0 and L.xeq_message_wq_first_table(WQ, 0, 0, 0) == 0      # T > 128, no table
    assert L.xeq_message_wq_first_table(WQ, 87, 1, 0) == 0                        # training mode
    assert L.xeq_message_wq_first_table(WQ, 87, 0, 1) == 0                        # per-node front (charge / spin embedding)
    assert L.xeq_message_wq_first_table(SB, 87, 0, 0) == 0 and L.xeq_message_wq_first_table(GENERIC, 87, 0, 0) == 0
    monkeypatch.setenv("XEQ_WQ_FIRST_TABLE", "0")
    assert L.xeq_message_wq_first_table(WQ, 87, 0, 0) == 0
