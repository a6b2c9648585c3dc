"""Round-5 kernels that collapse the small launches of a step (pytest -m gpu): the fused energy head with its saved reverse row, the
first message block's front half as one gather, degrees -> guarded row pointer in one launch, and one edge-gradient launch for all
message blocks.  Each against a float64 / integer restatement of the same arithmetic (nn/output.py:104-128, nn/xpainn.py:62-81,
128-139, data/transform.py:58-64, nn/basic.py:143-159)."""
import numpy as np
import pytest
import torch

from xequinet_amd.data import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"


# (32, 32): k-split halves of two k-groups, shorter than the weight prefetch; (128, 96): three hidden tiles, no k split; the 256-wide
# heads need more than the default 64 KB of dynamic LDS (67 072 and 99 840 bytes)
@pytest.mark.parametrize("node_dim,hidden_dim", [(128, 64), (32, 32), (128, 96), (256, 128), (256, 256)])
def test_fused_head_energies_and_saved_reverse_row(node_dim, hidden_dim):
    """Every width meets 3e-6 max(1, |ref|).  Measured on one MI355X (kernel | an ATen f32 evaluation of the same Sequential, both against
    the f64 restatement; atomic, total, g_s, g_s of the summed energies):
      (128, 64)   1.2e-7 2.3e-7 4.6e-8 2.3e-8 | 1.1e-7 3.9e-7 3.7e-8 3.0e-8      (32, 32)    6.1e-8 7.8e-8 4.9e-8 1.5e-8 | 7.8e-8 8.4e-8 4.4e-8 1.8e-8
      (128, 96)   1.3e-7 4.1e-7 4.7e-8 2.2e-8 | 1.6e-7 4.1e-7 3.7e-8 2.4e-8      (256, 128)  2.0e-7 4.4e-7 3.9e-8 2.3e-8 | 1.9e-7 3.5e-7 3.8e-8 2.4e-8
      (256, 256)  1.4e-7 2.9e-7 4.4e-8 2.9e-8 | 2.2e-7 5.1e-7 7.7e-8 2.6e-8"""
    from xequinet_amd.nn.fused import EnergyReadout
    from xequinet_amd.nn.output import EnergyOut

    torch.manual_seed(0)
    head = EnergyOut(node_dim=node_dim, hidden_dim=hidden_dim).to(DEV)
    n_per = [3, 17, 0, 29, 1, 40]
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(n_per)]), device=DEV)
    batch = torch.repeat_interleave(torch.arange(len(n_per), device=DEV), torch.tensor(n_per, device=DEV))
    n = int(ptr[-1])
    s = torch.randn(n, node_dim, device=DEV, requires_grad=True)
    assert EnergyReadout.supported(head.out_mlp, s)
    atomic, total = EnergyReadout.apply(s, head.out_mlp, batch, ptr)
    # float64 restatement
    import copy

    ref = copy.deepcopy(head.out_mlp).double()
    s64 = s.detach().double().requires_grad_()
    a64 = ref(s64).reshape(-1)
    t64 = torch.zeros(len(n_per), dtype=torch.float64, device=DEV).index_add(0, batch, a64)

    def close(name, got, want):
        err, bound = float((got.detach().double() - want.detach()).abs().max()), 3e-6 * max(1.0, float(want.detach().abs().max()))
        print(f"head ({node_dim}, {hidden_dim}) {name}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, err, bound)

    close("atomic", atomic, a64)
    close("total", total, t64)
    # reverse pass for gradients at both outputs, one of them a broadcast scalar (what the sum of the energies hands over)
    ga = torch.randn(n, device=DEV)
    gt = torch.full((len(n_per),), -1.0, device=DEV)
    (g,) = torch.autograd.grad([atomic, total], s, [ga, gt])
    (g64,) = torch.autograd.grad([a64, t64], s64, [ga.double(), gt.double()], retain_graph=True)
    close("g_s", g, g64)
    (g1,) = torch.autograd.grad(EnergyReadout.apply(s, head.out_mlp, batch, ptr)[1].sum(), s)
    (g1_64,) = torch.autograd.grad(t64.sum(), s64)
    close("g_s of the summed energies", g1, g1_64)
    # rows do not depend on the batch they sit in
    a_half, _ = EnergyReadout.apply(s[:20].detach(), head.out_mlp, batch[:20], torch.tensor([0, 3, 20], device=DEV))
    assert torch.equal(a_half, atomic[:20].detach())


def test_first_block_front_is_the_three_gathers():
    from xequinet_amd.nn import resolve_model
    from xequinet_amd.nn.fused import first_block_front

    torch.manual_seed(1)
    model = resolve_model("xpainn").eval().requires_grad_(False).to(DEV)
    emb, msg = model.mods["embedding"], model.mods["message_0"]
    for dt in (torch.int32, torch.int64):
        z = torch.tensor([1, 6, 8, 1, 9, 7, 6, 0, 86], device=DEV, dtype=dt)
        rows = emb._embedded_rows(z)
        s, h, xhat = first_block_front(msg, z, rows, z.shape[0])
        _, (h_t, x0_t) = msg._element_front
        assert torch.equal(s, rows.index_select(0, z.long()))
        assert torch.equal(h, h_t.index_select(0, z.long()))
        n, F = z.shape[0], 128
        assert torch.equal(xhat[: n * F].view(n, F), x0_t.index_select(0, z.long())) and float(xhat[n * F :].abs().max()) == 0.0


@pytest.mark.parametrize("n", [0, 1, 63, 1024, 1025, 18609, 36864])
def test_degrees_to_guarded_row_pointer_in_one_launch(n):
    from xequinet_amd import lib
    from xequinet_amd.lib import call, ptr, stream

    g = torch.Generator().manual_seed(n)
    deg = torch.randint(0, 40, (n,), generator=g, dtype=torch.int32).to(DEV)
    want = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(deg.long(), 0)]).to(torch.int32)
    total = int(want[-1])
    for cap, empty in ((-1, False), (total, False), (total - 1, total > 0)):
        rowptr = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
        count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        run = torch.full((1,), 5, dtype=torch.int64, device=DEV)
        call("xeq_rowptr_from_degrees", ptr(deg), n, cap, ptr(rowptr), ptr(count), ptr(run), stream())
        assert int(count) == total and int(run) == total + 5
        assert torch.equal(rowptr, torch.zeros_like(want) if empty else want)
    assert lib.load().xeq_rowptr_from_degrees_max() >= 32768


def test_one_edge_gradient_launch_for_all_blocks_equals_one_per_block():
    """The model's forces with the deferral (one xeq_message_wq_edge_grad_sum) against the same model with one edge-gradient launch
    per block and autograd's sums: the same arithmetic up to the association of three float additions."""
    from xequinet_amd import ops
    from xequinet_amd.data import NeighborTransform, XequiBatch
    from xequinet_amd.nn import resolve_model

    torch.manual_seed(0)
    model = resolve_model("xpainn").eval().requires_grad_(False).to(DEV)
    pos, z, ptr = syn.synth_qm9_batch(400, seed=5)     # above the wq kernels' minimum edge count
    b = NeighborTransform(5.0)(XequiBatch(torch.tensor(pos, dtype=torch.float32, device=DEV), torch.tensor(z, device=DEV), torch.tensor(ptr, device=DEV)))
    with torch.enable_grad():
        out = model(b.to_dict(), compute_forces=True)
    orig = ops.EdgeGradDeferral.register
    ops.EdgeGradDeferral.register = lambda self: False      # nobody registers: every block launches its own edge gradient
    try:
        with torch.enable_grad():
            ref = model(b.to_dict(), compute_forces=True)
    finally:
        ops.EdgeGradDeferral.register = orig
    assert torch.equal(out["energy"], ref["energy"])
    scale = float(ref["forces"].abs().max())
    assert float((out["forces"] - ref["forces"]).abs().max()) <= 2e-6 * max(1.0, scale)
    assert not torch.equal(out["forces"], torch.zeros_like(out["forces"]))
