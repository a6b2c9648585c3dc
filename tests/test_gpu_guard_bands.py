"""Guard bands (tests/guard_bands.py) over the real kernels: where a kernel writes, and whether what lies behind a buffer reaches a result.

1. whole evaluations with every device allocation of the Python front on a guarded tensor: the same bits as the plain evaluation run
   just before, finite, all bands intact (a ``torch.empty`` body starts as NaN: an element a kernel should have written and did not
   shows up as a mismatch or a non-finite number);
2. one training step (native parameter-gradient pass; the twice-differentiable force-loss pass) likewise;
3. entry points one by one at ragged sizes, inputs and outputs guarded, once with finite garbage in the bands and once with NaN: the
   outputs agree bit for bit (no read past the end reaches a result), hold no never-written element, and no band changed;
4. a positive control: a real kernel told to write one row more than its output holds is caught.
Captured (HIP-graph) paths issue the same launches and are not interposed."""
import os

import numpy as np
import pytest
import torch

from oracle import xpainn_oracle as orc
from tests import guard_bands as gb
from tests.test_gpu_small_rows import _forms
from xequinet_amd import keys, lib
from xequinet_amd.data import NeighborTransform, XequiBatch
from xequinet_amd.data import synthetic as syn

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129, 333]
MUL = (128, 64, 32)
IRREPS = "128x0e + 64x1o + 32x2e"
F, C, D = 128, 224, 480


def _bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------ 1. whole evaluations
def _evaluate(model, pos, z, ptr, dtype=torch.float32, virial=False, extra=None, cutoff=5.0, data=None):
    """NeighborTransform + model, eager: the neighbour list, the edge views and every block allocate inside the caller's net."""
    if data is None:
        b = XequiBatch(torch.tensor(pos, dtype=dtype), torch.tensor(z), torch.tensor(ptr), **(extra or {})).to(DEV)
        data = NeighborTransform(cutoff)(b).to_dict()
    with torch.enable_grad():
        out = model(dict(data), compute_forces=True, compute_virial=virial)
    return {k: out[k].detach().clone() for k in ("energy", "forces") + (("virial",) if virial else ())}


def _plain_then_guarded(fn):
    plain = fn()
    torch.cuda.synchronize()
    with gb.guard_allocations() as net:
        got = fn()
    assert net.count > 10, "the interposer saw no allocation"
    for k, v in plain.items():
        assert torch.isfinite(got[k]).all(), k
        assert _same_bits(got[k], v), f"{k}: {float((got[k] - v).abs().max()):.3e}"
    return net


def _lone_atom_batch():
    pos, z, ptr = syn.synth_qm9_batch(4, seed=2)      # the batch of test_model_batch_with_lone_atoms_through_neighbor_transform
    cut = int(ptr[2])
    pos = np.concatenate([pos[:cut], [[50.0, 50.0, 50.0]], pos[cut:]])
    z = np.concatenate([z[:cut], [8], z[cut:]])
    ptr = np.concatenate([ptr[:3], ptr[2:] + 1])
    pos[0] += 200.0
    return pos, z, ptr


def _node_block_batches():
    """(first batch of whole molecules that takes the fused node-block path, the largest one below it), sized from the library."""
    auto = lib.load().xeq_node_block_auto
    pos, z, ptr = syn.synth_qm9_batch(1200, seed=9)
    g = next(g for g in range(1, len(ptr)) if auto(int(ptr[g])))
    assert g > 1 and not auto(int(ptr[g - 1]))
    cut = lambda g: (pos[:int(ptr[g])], z[:int(ptr[g])], ptr[:g + 1])
    return cut(g), cut(g - 1)


@pytest.mark.parametrize("system", ["aspirin", "qm9_16", "lone_atoms", "one_atom", "node_block", "below_node_block", "aspirin_f64"])
def test_whole_evaluation_under_guard_bands(system):
    from tests.test_gpu_parity import _build

    dtype = torch.float64 if system.endswith("f64") else torch.float32
    model, _ = _build(dtype)
    if system.startswith("aspirin"):
        pos, z, ptr = syn.synth_aspirin()
    elif system == "qm9_16":
        pos, z, ptr = syn.synth_qm9_batch(16, seed=4)
    elif system == "lone_atoms":
        pos, z, ptr = _lone_atom_batch()
    elif system == "one_atom":
        pos, z, ptr = np.array([[0.0, 0.0, 0.0]]), np.array([6]), np.array([0, 1])
    else:
        big, small = _node_block_batches()
        pos, z, ptr = big if system == "node_block" else small
    n0 = lib.launch_count()
    _plain_then_guarded(lambda: _evaluate(model, pos, np.asarray(z).astype(np.int32), ptr, dtype))
    if system in ("node_block", "below_node_block"):
        assert ("xeq_node_block_fwd" in lib.launch_names(n0)) == (system == "node_block")


def test_periodic_water_box_with_virial_under_guard_bands():
    from tests.test_gpu_parity import _build

    model, _ = _build(torch.float32)
    f = np.load(os.path.join(GOLDEN, "radius_graph_pbc_water192.npz"))
    _, z, ptr, _ = syn.synth_water_box(4, seed=5)
    t = lambda a, dt=None: torch.tensor(a, device=DEV, dtype=dt)
    data = {"pos": t(f["pos"], torch.float32), "atomic_numbers": t(z.astype(np.int32)), "edge_index": t(f["edge_index"]), "ptr": t(ptr),
            "batch": t(np.zeros(len(z), dtype=np.int64)), "cell": t(f["cell"], torch.float32), "cell_offsets": t(f["cell_offsets"], torch.float32)}
    _plain_then_guarded(lambda: _evaluate(model, None, None, None, virial=True, data=data))


def test_charged_spin_model_under_guard_bands():
    from tests.test_gpu_electronic import _batch, _model

    model = _model(1).to(DEV).eval().requires_grad_(False)
    pos, z, ptr = syn.synth_qm9_batch(16, seed=3)
    rng = np.random.default_rng(0)
    charge, spin = rng.integers(-2, 3, size=16), rng.integers(0, 3, size=16)
    n0 = lib.launch_count()
    _plain_then_guarded(lambda: _evaluate(model, None, None, None, data=_batch(pos, z, ptr, model.cutoff_radius, charge=charge, spin=spin).to_dict()))
    assert lib.launch_names(n0).count("xeq_electronic_mix") == 4


@pytest.mark.parametrize("impl", ["generic", "sb", "wq"])
def test_message_kernel_families_under_guard_bands(impl, monkeypatch):
    from tests.test_gpu_parity import _build

    monkeypatch.setenv("XEQ_MESSAGE_IMPL", impl)
    model, _ = _build(torch.float32)
    pos, z, ptr = syn.synth_qm9_batch(40, seed=8)
    n0 = lib.launch_count()
    _plain_then_guarded(lambda: _evaluate(model, pos, z.astype(np.int32), ptr))
    name = {"generic": "xeq_message_fwd", "sb": "xeq_message_fwd_sb", "wq": "xeq_message_fwd_wq"}[impl]
    assert any(n.startswith(name) and (impl != "generic" or n == name) for n in lib.launch_names(n0))


# ------------------------------------------------------------------------------------------------------- 2. one training step
@pytest.mark.parametrize("case", ["energy", "energy+forces"])
def test_training_step_under_guard_bands(case):
    """Energy loss: the native parameter-gradient pass of nn/training.py on a small batch (it owns the *_parts / *_chunks partial
    buffers, sized by library functions).  Energy + force loss on 3 molecules: the twice-differentiable pass."""
    from tests.test_gpu_training import _batch, _model, _targets
    from xequinet_amd import train
    from xequinet_amd.nn import training as tr

    forces = "forces" in case
    model = _model(torch.float32, action_blocks=3).train()
    host, dev = _batch(3 if forces else 16, 5, torch.float32)
    tgt = {k: (v.float() if v.is_floating_point() else v).to(DEV) for k, v in _targets(host, 7, False).items()}
    weights = {keys.TOTAL_ENERGY: 1.0, **({keys.FORCES: 10.0} if forces else {})}

    def step():
        model.zero_grad(set_to_none=True)
        data = dict(dev)
        loss, _ = train.weighted_loss(model(data, forces, False), tgt, weights)
        loss.backward()
        assert bool(data[tr.PARAM_GRADS]) == (not forces)
        out = {"loss": loss.detach().clone()}
        out.update({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
        return out

    # What "the plain run" is has to be settled first.  The twice-differentiable pass scatters through ATen (atomics: measured on the
    # MI355X, two plain steps differ in 73 of 77 tensors, up to 1.1e-5 in message_0.rbf_lin.bias), so it runs with torch's deterministic
    # algorithms; and even then the first two steps of a process give other bits than every later one (1.9e-6 in embedding.1.weight, the
    # same values each time, plain or guarded), so three steps run first and two plain steps are required to agree before the guarded one.
    det = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        for _ in range(3):
            step()
        first, again = step(), step()
        moved = {k: float((again[k] - first[k]).abs().max()) for k in first if not _same_bits(again[k], first[k])}
        assert not moved, f"two plain steps differ: {moved}"
        _plain_then_guarded(step)
    finally:
        torch.use_deterministic_algorithms(det[0], warn_only=det[1])


# --------------------------------------------------------------------------------------- 3. entry points, inputs and outputs guarded
def _banded(fn, inputs, forms=None):
    """``fn(*inputs)`` -> tensors, with every tensor of ``inputs`` copied into a guarded one and every allocation ``fn`` makes guarded,
    once with finite-garbage bands and once with NaN bands."""
    res = {}
    for fill in ("finite", "nan"):
        ins = [gb.guarded_copy(t, fill) if isinstance(t, torch.Tensor) else t for t in inputs]
        with gb.guard_allocations(fill=fill) as net:
            out = fn(*ins)
        assert net.count > 0
        gb.check(*[t for t in ins if isinstance(t, torch.Tensor)])
        res[fill] = [o for o in out if o is not None]
    assert len(res["finite"]) == len(res["nan"]) > 0
    for i, (a, b) in enumerate(zip(res["finite"], res["nan"])):
        if a.element_size() in (4, 8):
            assert not gb.unwritten(a).any() and not gb.unwritten(b).any(), f"output {i}: {int(gb.unwritten(b).sum())} elements never written"
        if a.is_floating_point():
            assert torch.isfinite(b).all(), f"output {i} is not finite with NaN bands"
        assert _same_bits(a, b), f"output {i} depends on what lies behind a buffer"
    return res["nan"]


def _rand(*shape, seed=0, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed + sum(shape))
    return torch.randn(*shape, device=DEV, generator=g, dtype=dtype)


@pytest.mark.parametrize("small", [0, 1 << 40])
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_linear_fwd_guarded(n, gather, small):
    from xequinet_amd.nn import fused

    torch.manual_seed(1)
    lin = torch.nn.Linear(56, 128).to(DEV)
    pack = fused._linear_pack(lin, lin.weight, lin.bias, False)
    x = _rand(n if not gather else 20, 56)
    idx = torch.randint(0, 20, (n,), device=DEV, dtype=torch.int32) if gather else None
    with _forms(small):
        y, pre = _banded(lambda x, idx: fused._linear(x, pack, 56, 128, True, act=1, row_index=idx, want_pre=True), [x, idx])
    rows = x if idx is None else x[idx.long()]
    ref = torch.nn.functional.linear(rows.double(), lin.weight.double(), lin.bias.double())
    assert (pre.double() - ref).abs().max() <= 1e-4 * (1.0 + ref.abs().max())


@pytest.mark.parametrize("small", [0, 1 << 40])
@pytest.mark.parametrize("n", SIZES)
def test_mlp2_fwd_bwd_guarded(n, small):
    from xequinet_amd.nn import fused

    torch.manual_seed(2)
    seq = torch.nn.Sequential(torch.nn.Linear(128, 128), torch.nn.SiLU(), torch.nn.Linear(128, 576)).to(DEV).requires_grad_(False)
    fused._mlp_packs(seq)
    with _forms(small):
        pre, y = _banded(lambda x: fused._mlp_fwd(seq, x), [_rand(n, 128)])
        (gx,) = _banded(lambda g, pre: (fused._mlp_bwd(seq, g, pre),), [_rand(n, 576, seed=1), pre])
    assert pre.shape == (n, 128) and y.shape == (n, 576) and gx.shape == (n, 128)


@pytest.mark.parametrize("small", [0, 1 << 40])
@pytest.mark.parametrize("n", SIZES)
def test_update_block_guarded(n, small):
    """xeq_update_uv_fwd / _bwd, xeq_norm_bwd, the update MLP with dot_lin and their reverse (fused.UpdateBlock), both forms."""
    from xequinet_amd.nn import fused
    from xequinet_amd.nn.xpainn import XPainnUpdate

    torch.manual_seed(n)
    blk = XPainnUpdate(node_dim=F, node_irreps=IRREPS).to(DEV).eval().requires_grad_(False)

    def run(s, x, gs, gx):
        s, x = s.requires_grad_(True), x.requires_grad_(True)
        with torch.enable_grad():
            so, xo = fused.UpdateBlock.apply(s, x, blk)
            g = torch.autograd.grad([so, xo], [s, x], [gs, gx])
        return so.detach(), xo.detach(), g[0], g[1]

    run(_rand(4, F), _rand(4, D), _rand(4, F), _rand(4, D))     # packed weights: outside the net
    n0 = lib.launch_count()
    with _forms(small):
        _banded(run, [_rand(n, F), _rand(n, D), _rand(n, F, seed=1), _rand(n, D, seed=1)])
    names = lib.launch_names(n0)
    assert "xeq_update_uv_fwd" in names and "xeq_update_uv_bwd" in names


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", SIZES)
def test_norm_fwd_bwd_guarded(n, dtype):
    from xequinet_amd.nn import fused
    from xequinet_amd.nn.xpainn import XPainnMessage

    torch.manual_seed(3)
    msg = XPainnMessage(node_dim=F, node_irreps=IRREPS).to(dtype).to(DEV).requires_grad_(False)
    s, x = _rand(n, F, dtype=dtype), _rand(n, D, dtype=dtype)
    shat, xhat, stats = _banded(lambda s, x: fused._norm_fwd(s, x, msg.norm, msg.o3norm, F, MUL)[:3], [s, x])
    assert shat.shape == (n, F) and xhat.numel() == n * D and stats.shape == (n, 4)
    args = [s, x, stats, _rand(n, F, seed=1, dtype=dtype), _rand(n * D, seed=1, dtype=dtype), _rand(n, F, seed=2, dtype=dtype), _rand(n, D, seed=2, dtype=dtype)]
    _banded(lambda s, x, stats, g_shat, g_xhat, res_s, res_x: fused._norm_bwd(s, x, msg.norm, msg.o3norm, stats, 1, F, MUL, g_shat, F, g_xhat, res_s, res_x), args)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", SIZES)
def test_eqln_sph_harm_radial_guarded(n, dtype):
    """xeq_eqln_fwd / _bwd, xeq_sph_harm_fwd / _bwd, xeq_radial_fwd."""
    from xequinet_amd import ops

    w, b = 1.0 + 0.1 * _rand(C, dtype=dtype), 0.1 * _rand(MUL[0], dtype=dtype)

    def eqln(x, g):
        x = x.requires_grad_(True)
        with torch.enable_grad():
            y = ops.EqLayerNorm.apply(x, w, b, MUL, 1e-5)
            (gx,) = torch.autograd.grad(y, x, g)
        return y.detach(), gx

    _banded(eqln, [_rand(n, D, dtype=dtype), _rand(n, D, seed=1, dtype=dtype)])

    def sph(v, g):
        v = v.requires_grad_(True)
        with torch.enable_grad():
            y = ops.SphHarm.apply(v, MUL, True)
            (gv,) = torch.autograd.grad(y, v, g)
        return y.detach(), gv

    _banded(sph, [_rand(n, 3, dtype=dtype), _rand(n, D, seed=1, dtype=dtype)])
    freq = (torch.arange(1, 21, device=DEV, dtype=dtype) * (np.pi / 5.0))
    rbf, fcut = _banded(lambda d, p0: ops.radial_basis(d, "bessel", "cosine", 20, 5.0, p0), [0.5 + 4.0 * torch.rand(n, device=DEV, dtype=dtype), freq])
    assert rbf.shape == (n, 20) and fcut.shape == (n,)


@pytest.mark.parametrize("n", SIZES)
def test_head_and_segment_sum_guarded(n):
    """xeq_head_fwd, xeq_segment_sum (width 1 inside the head; width 9 on its own), xeq_head_bwd: n nodes in ragged graphs, one empty."""
    from xequinet_amd import ops
    from xequinet_amd.nn import fused

    torch.manual_seed(4)
    seq = torch.nn.Sequential(torch.nn.Linear(F, 64), torch.nn.SiLU(), torch.nn.Linear(64, 1)).to(DEV).requires_grad_(False)
    ptr = torch.tensor(sorted({0, n // 3, (2 * n) // 3, n}) + [n], device=DEV)      # ragged graphs; the last one is empty
    batch = torch.repeat_interleave(torch.arange(ptr.numel() - 1, device=DEV), ptr[1:] - ptr[:-1])
    s = _rand(n, F)
    assert fused.EnergyReadout.supported(seq, s)
    fused.EnergyReadout.apply(s.clone().requires_grad_(True), seq, batch, ptr)          # packed weights: outside the net

    def head(s, batch, ptr, g_atomic, g_total):
        s = s.requires_grad_(True)
        with torch.enable_grad():
            atomic, total = fused.EnergyReadout.apply(s, seq, batch, ptr)
            (gs,) = torch.autograd.grad([atomic, total], s, [g_atomic, g_total])
        return atomic.detach(), total.detach(), gs

    atomic, total, _ = _banded(head, [s, batch, ptr, _rand(n), _rand(ptr.numel() - 1, seed=1)])
    assert float(total[-1]) == 0.0 and abs(float(total.sum() - atomic.sum())) <= 1e-3 * (1.0 + float(atomic.abs().sum()))
    for dtype in (torch.float32, torch.float64):
        (out,) = _banded(lambda src, ptr: (ops.SegmentSum.apply(src, ptr),), [_rand(n, 9, dtype=dtype), ptr])
        assert out.shape == (ptr.numel() - 1, 9) and not out[-1].any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", SIZES)
def test_edge_vectors_guarded(n, dtype):
    """xeq_edge_vectors_fwd / _bwd on n edges between 40 atoms (atoms 37 .. 39 have no edge); the edge views are built inside the net."""
    from xequinet_amd import ops

    g = torch.Generator().manual_seed(n)
    c = torch.randint(0, 37, (n,), generator=g)
    nb = (c + 1 + torch.randint(0, 36, (n,), generator=g)) % 37
    ei = torch.stack([c, nb]).to(DEV)

    def run(pos, ei, gvec):
        graph = ops.EdgeGraph(ei, 40)
        pos = pos.requires_grad_(True)
        with torch.enable_grad():
            vec, dist = ops.EdgeVectors.apply(pos, graph, None, None, None)
            (gp,) = torch.autograd.grad(vec, pos, gvec)
        return vec.detach(), dist.detach(), gp

    pos = 3.0 * _rand(40, 3, dtype=dtype)
    vec, dist, gp = _banded(run, [pos, ei, _rand(n, 3, seed=1, dtype=dtype)])
    assert torch.equal(vec, pos[ei[0]] - pos[ei[1]]) and not gp[37:].any()


@pytest.mark.parametrize("kind", ["charge", "spin"])
@pytest.mark.parametrize("n", SIZES)
def test_electronic_fwd_guarded(n, kind):
    from tests.electronic_oracle import electronic
    from xequinet_amd.nn.electronic import ChargeEmbedding, SpinEmbedding

    torch.manual_seed(5)
    mod = (ChargeEmbedding if kind == "charge" else SpinEmbedding)(node_dim=F).to(DEV).eval().requires_grad_(False)
    cuts = sorted({0, 1 if n > 1 else 0, n // 2, n})
    ptr = torch.tensor(cuts, device=DEV)
    total = torch.tensor(([2.0, -1.0, 3.0, -2.0] if kind == "charge" else [1.0, 2.0, 0.0, 3.0])[:len(cuts) - 1], device=DEV)
    s = _rand(n, F)
    mod._kernel_form(s, total, ptr)     # packed weights: outside the net
    (out,) = _banded(lambda s, total, ptr: (mod._kernel_form(s, total, ptr),), [s, total, ptr])
    batch = torch.repeat_interleave(torch.arange(len(cuts) - 1, device=DEV), ptr[1:] - ptr[:-1])
    ref = electronic(s.double().cpu(), batch.cpu(), total.double().cpu(), {k: v.double().cpu() for k, v in mod.state_dict().items()}, kind)
    out = out.cpu()
    assert float((out.double() - ref).abs().max()) <= 2e-6 * float(ref.abs().max())


@pytest.mark.parametrize("mode", ["tail", "gx", "last"])
@pytest.mark.parametrize("n", SIZES)
def test_node_block_fwd_bwd_guarded(n, mode):
    """xeq_node_block_fwd / _bwd through nn/nodeblock.py: its internal tensors are whole workgroups of rows (xeq_node_block_rows)."""
    from tests.test_gpu_nodeblock import _modules
    from xequinet_amd.nn import nodeblock

    upd, msg = _modules(11)
    upd, msg = upd.to(DEV), msg.to(DEV)
    tail = mode == "tail"
    m = msg if tail else None
    nodeblock.packed_fwd(upd, m), nodeblock.packed_bwd(upd, m, with_gx=mode != "last")     # weight programs: outside the net

    def run(s, x, g_s, g_x, g_h, g_xh):
        o = nodeblock.node_block_fwd(s, x, upd, m, want_x=True)
        gs, gx = nodeblock.node_block_bwd(o, s, x, upd, m, g_s, g_x, g_h, g_xh)
        return [o["s_out"], o["x_out"], o["stats"], gs, gx] + ([o["h2"], o["xhat2"], o["stats2"]] if tail else [])

    ins = [_rand(n, F), _rand(n, D), _rand(n, F, seed=1), _rand(n, D, seed=1) if mode != "last" else None,
           _rand(n, F + 2 * C, seed=2) if tail else None, _rand(n * D, seed=2) if tail else None]
    _banded(run, ins)


@pytest.mark.parametrize("impl", ["wq", "sb", "generic"])
@pytest.mark.parametrize("n_mol,lone", [(1, 0), (1, 2), (2, 3), (5, 4), (9, 7)])
def test_message_fwd_bwd_guarded(n_mol, lone, impl, monkeypatch):
    """xeq_message_fwd_wq / _bwd_wq, _sb and the generic form through ops.message_forward / message_backward on a small ragged graph
    with isolated nodes; the edge count is made odd, so the last quad of the wq walk and the last stream are partial."""
    from xequinet_amd import ops

    monkeypatch.setenv("XEQ_MESSAGE_IMPL", impl)
    rng = np.random.default_rng(n_mol)
    pos, z, ptr = syn.synth_qm9_batch(n_mol, seed=30 + n_mol)
    ei = orc.radius_graph_canonical(pos.astype(np.float32), ptr, 4.0)
    E = ei.shape[1] - (1 - ei.shape[1] % 2)
    ei = ei[:, :E]
    N = len(pos) + lone                                              # the isolated nodes sit behind the last molecule
    assert E % 2 == 1 and (np.bincount(ei[0], minlength=N) % 4 != 0).any()
    B = 20
    H = F + 2 * C
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)
    vec = t(pos[ei[0]] - pos[ei[1]])
    W, b = t(rng.normal(size=(H, B)) / np.sqrt(B)), t(rng.normal(size=H))
    p0 = t(np.pi * np.arange(1, B + 1) / 4.0)
    cfg = ("bessel", "cosine", B, 4.0, F, MUL)
    ops.wq_packed_weights(W, b, B, F, MUL)

    def run(h, xhat, vec, s, x, ei, g_s, g_x):
        graph = ops.EdgeGraph(ei, N)
        s_out, x_out, saved, used = ops.message_forward(h, xhat, vec, s, x, W, b, p0, None, graph, cfg, want_backward=True)
        assert used == impl
        g_h, g_xhat, g_vec, _, _ = ops.message_backward(saved, graph, cfg, used, g_s, g_x)
        return s_out, x_out, g_h, g_xhat, g_vec

    s, x = _rand(N, F), _rand(N, D)
    s_out, x_out, g_h, g_xhat, g_vec = _banded(run, [_rand(N, H, seed=1), _rand(N, D, seed=1), vec, s, x, torch.tensor(ei, device=DEV),
                                                     _rand(N, F, seed=2), _rand(N, D, seed=2)])
    if lone:
        assert torch.equal(s_out[-lone:], s[-lone:]) and torch.equal(x_out[-lone:], x[-lone:]) and not g_h[-lone:].any()


# ------------------------------------------------------------------------------------------------------- 4. positive control
def test_a_real_kernel_writing_one_row_too_many_is_caught():
    """xeq_segment_sum is told of G + 1 = 6 segments while its guarded output holds G = 5 rows of 64 floats.  Every address it touches is
    allocated: ptr really has G + 2 = 7 entries and the source all 36 rows they name (the sixth segment sums real numbers, so what
    is stored differs from the band's pattern); the kernel writes that segment's 64 x 4 = 256 B behind the end of the output, inside
    its 131 072 B back band, and nothing else.  The checker must name the back band of the output at offset 0.  One call."""
    ptr = torch.tensor([0, 4, 9, 9, 20, 33, 36], device=DEV)
    src = gb.guarded_copy(_rand(36, 64))
    out = gb.guarded((5, 64), torch.float32, DEV)
    assert gb.BAND_BYTES >= 256
    lib.call("xeq_segment_sum", lib.XEQ_F32, lib.ptr(src), lib.ptr(ptr), 6, 64, lib.ptr(out), lib.stream())
    torch.cuda.synchronize()
    gb.check(src)
    assert not gb.unwritten(out).any() and (out[2] == 0).all()
    with pytest.raises(gb.GuardViolation) as e:
        gb.check(out)
    assert e.value.side == "back" and e.value.offset == 0 and os.path.samefile(e.value.site.rsplit(":", 1)[0], __file__)
    again = gb.guarded((5, 64), torch.float32, DEV)                       # the same call with the right count leaves the bands alone
    lib.call("xeq_segment_sum", lib.XEQ_F32, lib.ptr(src), lib.ptr(ptr), 5, 64, lib.ptr(again), lib.stream())
    torch.cuda.synchronize()
    gb.check(again, src)
    assert torch.equal(again, out)
