"""Host side of the run-time-width MLP kernels (xeq_mlp2h_*, csrc/xeq_mlp.hip): the predicate table, what PaiNN's native form now
admits, and the POWER of the comparison tests/test_gpu_mlp_widths.py makes -- the f64 reference evaluated a second time with one
deliberate defect must move an output by at least 10 x the bound the GPU test uses for that output, or the bound could hide a wrong
kernel.  No GPU: the predicates are host logic of the built library."""
import pytest
import torch

from tests import mlp_width_cases as mc
from xequinet_amd import lib

POWER = 10.0


def test_predicate_table():
    L = lib.load()
    assert len(mc.SUPPORTED) == 24
    for k1, H, n2 in mc.SUPPORTED:
        assert L.xeq_mlp2h_supported(lib.XEQ_F32, k1, H, n2) == 1, (k1, H, n2)
        assert L.xeq_mlp2h_supported(lib.XEQ_F32, n2, H, k1) == 1, (n2, H, k1)      # the reverse pass's view of the same stack
    for what, dtype, k1, H, n2 in mc.REFUSED:
        assert L.xeq_mlp2h_supported(dtype, k1, H, n2) == 0, what
    # the 128-wide family keeps its envelope
    assert L.xeq_mlp2_supported(lib.XEQ_F32, 128, 64, 576) == 0
    assert L.xeq_mlp2_supported(lib.XEQ_F32, 128, 128, 576) == 1
    assert "xeq_mlp2h_fwd" in lib.EXPORTS and "xeq_mlp2h_bwd" in lib.EXPORTS


@pytest.mark.parametrize("F,native", [(32, True), (64, True), (256, True), (48, False)])
def test_painn_native_form_follows_the_new_predicate(F, native):
    from xequinet_amd.nn import painn, resolve_model

    assert painn.native_supported(resolve_model("painn", node_dim=F)) is native


def test_reference_is_the_module_and_its_autograd():
    c = mc.case(64, 128, 192, 33)
    seq = torch.nn.Sequential(torch.nn.Linear(128, 64), torch.nn.SiLU(), torch.nn.Linear(64, 192)).double()
    with torch.no_grad():
        for prm, v in zip((seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias), (c.w1, c.b1, c.w2, c.b2)):
            prm.copy_(v)
    x = c.x.clone().requires_grad_()
    y = seq(x)
    (gx,) = torch.autograd.grad(y, x, c.g)
    assert torch.allclose(y.detach(), c.ref["y"], rtol=0, atol=1e-12) and torch.allclose(gx, c.ref["gx"], rtol=0, atol=1e-12)
    assert torch.allclose(seq[0](c.x), c.ref["pre"], rtol=0, atol=1e-12)


def test_a_case_is_the_first_rows_of_its_master():
    a, b = mc.case(96, 192, 288, 17), mc.case(96, 192, 288, 65)
    for k in mc.OUTPUTS:
        assert torch.equal(a.ref[k], b.ref[k][:17]) and a.ref[k].dtype == torch.float64 and a.ref32[k].dtype == torch.float32


# (a wave owns hidden tiles w and w + 4 only from five tiles on: below 160 there is nothing to swap)
DEFECTS = [(H, m) for H in mc.WIDTHS for m in sorted(mc.MUTATIONS) if not (m == "swap_hidden_tiles" and H < 160)]


@pytest.mark.parametrize("H,mutation", DEFECTS)
def test_every_defect_moves_the_reference_by_ten_bounds(H, mutation):
    """On the committed inputs, at the smallest and the largest row count of the GPU sweep and both stacks."""
    for k1, n2 in mc.stacks(H):
        for n in (mc.ROWS[0], mc.ROWS[-1]):
            c = mc.case(H, k1, n2, n)
            bad = mc.evaluate(c, torch.float64, mutation)
            for k in mc.MUTATIONS[mutation]:
                moved, bnd = float((bad[k] - c.ref[k]).abs().max()), mc.bound(c.ref[k], c.ref32[k])
                assert moved >= POWER * bnd, (H, k1, n2, n, mutation, k, moved, bnd)
