"""The two-layer MLP kernels at a run-time hidden width (xeq_mlp2h_fwd / _bwd, csrc/xeq_mlp.hip) through the C ABI and through
fused._mlp_fwd / _mlp_bwd, at every new width, against the f64 reference of tests/mlp_width_cases.py.

Every input sits between NaN guard bands, every output is handed over holding the never-written pattern between bands of its own, with
three rows more than the call is asked to fill: afterwards the bands are compared bit for bit, the n rows hold no never-written word and
the rows past n hold nothing else.

Bound per output tensor: max(1e-4 max(1, max|ref|), 1.5 err32), err32 the distance of the f32 restatement on the CPU from the f64
reference on the rows of the case.  tests/test_mlp_width_cases_host.py shows that every defect of its list moves the reference by at
least 10 x that bound.  The reverse pass is handed the pre-activation the forward kernel saved, as the model does."""
import pytest
import torch

from tests import guard_bands as gb, mlp_width_cases as mc
from xequinet_amd import lib
from xequinet_amd.lib import call, ptr, stream
from xequinet_amd.nn import fused

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPARE_ROWS = 3


def _in(t):
    return gb.guarded_copy(torch.as_tensor(t).to(torch.float32).to(DEV).contiguous())


def _out(*shape):
    return gb.guarded(shape, torch.float32, DEV, body="unwritten")


_PACKS = {}


def _packs(H, k1, n2):
    """(W1, W2, W2^T, W1^T) in fragment order, as fused._mlp_packs makes them, between bands; once per stack."""
    if (H, k1, n2) not in _PACKS:
        m = mc.master(H, k1, n2)
        w1, b1, w2, b2 = _in(m.w1), _in(m.b1), _in(m.w2), _in(m.b2)
        floats = lambda n_out, k_in: int(lib.load().xeq_mlp_packed_floats(n_out, k_in))
        out = []
        for w, b, n_out, k_in, tr in ((w1, b1, H, k1, 0), (w2, b2, n2, H, 0), (w2, None, H, n2, 1), (w1, None, k1, H, 1)):
            p = _out(floats(n_out, k_in))
            call("xeq_mlp_pack", ptr(w), ptr(b), n_out, k_in, tr, ptr(p), stream())
            out.append(p)
        torch.cuda.synchronize()
        gb.check(w1, b1, w2, b2, *out)
        assert not any(bool(gb.unwritten(p).any()) for p in out)
        _PACKS[(H, k1, n2)] = tuple(out)
    return _PACKS[(H, k1, n2)]


def _finish(inputs, outputs, n):
    torch.cuda.synchronize()
    gb.check(*inputs, *outputs)
    for t in outputs:
        assert not bool(gb.unwritten(t[:n]).any()), ("unwritten", tuple(t.shape), int(gb.unwritten(t[:n]).sum()))
        assert bool(gb.unwritten(t[n:]).all()), ("a row past n was written", tuple(t.shape))


def _run(H, k1, n2, x, g, n=None):
    """forward then reverse on the first n rows of x [., k1] / g [., n2] (CPU tensors) -> pre, y, gx (n rows each, on the CPU)"""
    n = x.shape[0] if n is None else n
    pk = _packs(H, k1, n2)
    xd, gd = _in(x[:n]), _in(g[:n])
    pre, y, gx = _out(n + SPARE_ROWS, H), _out(n + SPARE_ROWS, n2), _out(n + SPARE_ROWS, k1)
    call("xeq_mlp2h_fwd", lib.XEQ_F32, ptr(xd), k1, n, k1, H, ptr(pk[0]), ptr(pk[1]), n2, ptr(pre), ptr(y), n2, stream())
    _finish([xd, *pk], [pre, y], n)
    pre_in = _in(pre[:n].clone())
    call("xeq_mlp2h_bwd", lib.XEQ_F32, ptr(gd), n2, n, n2, H, ptr(pk[2]), ptr(pre_in), ptr(pk[3]), k1, ptr(gx), k1, stream())
    _finish([gd, pre_in, *pk], [gx], n)
    return {"pre": pre[:n].cpu(), "y": y[:n].cpu(), "gx": gx[:n].cpu()}


def _compare(c, got, tag):
    failed = []
    for k in mc.OUTPUTS:
        assert torch.isfinite(got[k]).all(), (tag, k)
        err, bnd = float((got[k].double() - c.ref[k]).abs().max()), mc.bound(c.ref[k], c.ref32[k])
        print(f"mlp2h {tag} {k}: err {err:.3e} bound {bnd:.3e}")
        if not err <= bnd:
            failed.append((k, err, bnd))
    assert not failed, (tag, failed)


@pytest.mark.parametrize("stack", (0, 1))
@pytest.mark.parametrize("H", mc.WIDTHS)
def test_forward_and_reverse_against_the_f64_reference(H, stack):
    """PaiNN's two stacks at every new width; row counts around the 16- and 32-row edges, one row, more than one tile; at 32 and 256
    also one row count on each side of every point where the deal of row tiles to workgroups changes."""
    k1, n2 = mc.stacks(H)[stack]
    for n in mc.ROWS + (mc.THRESHOLD_ROWS if H in (32, 256) else ()):
        c = mc.case(H, k1, n2, n)
        _compare(c, _run(H, k1, n2, c.x, c.g), f"H={H} k1={k1} n2={n2} n={n}")


def _seq(H, k1, n2):
    m = mc.master(H, k1, n2)
    seq = torch.nn.Sequential(torch.nn.Linear(k1, H), torch.nn.SiLU(), torch.nn.Linear(H, n2))
    with torch.no_grad():
        for prm, v in zip((seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias), (m.w1, m.b1, m.w2, m.b2)):
            prm.copy_(v.float())
    return seq.to(DEV).requires_grad_(False)


@pytest.mark.parametrize("H", (32, 96, 256))
def test_the_module_front_runs_the_kernels_and_takes_strided_rows(H):
    """fused._mlp_fwd / _mlp_bwd on the module give the bits of the C calls; a wider buffer gives the bits of its contiguous copy."""
    k1, n2 = mc.stacks(H)[1]
    c = mc.case(H, k1, n2, 65)
    seq = _seq(H, k1, n2)
    first = lib.launch_count()
    wide = torch.full((65, k1 + 24), float("nan"), device=DEV)
    wide[:, :k1] = c.x.float().to(DEV)
    x = wide[:, :k1]
    pre, y = fused._mlp_fwd(seq, x)
    assert getattr(seq, "_xeq_mlp_pack", None) is not None, "the matrix-core path did not run"
    pre_c, y_c = fused._mlp_fwd(seq, x.contiguous())
    gx = fused._mlp_bwd(seq, c.g.float().to(DEV), pre)
    names = lib.launch_names(first)
    assert names == ["xeq_mlp_pack"] * 4 + ["xeq_mlp2h_fwd", "xeq_mlp2h_fwd", "xeq_mlp2h_bwd"], names
    assert torch.equal(pre, pre_c) and torch.equal(y, y_c)
    got = _run(H, k1, n2, c.x, c.g)
    assert torch.equal(pre.cpu(), got["pre"]) and torch.equal(y.cpu(), got["y"]) and torch.equal(gx.cpu(), got["gx"])


@pytest.mark.parametrize("H", mc.WIDTHS)
def test_a_rows_bits_do_not_depend_on_the_rows_around_it(H):
    """The first 45 rows alone, inside 300 rows and (32, 256) inside launches whose row tiles have one workgroup each (4 097 rows) or a
    shared last round (8 200): the same bits, forward and reverse."""
    k1, n2 = mc.stacks(H)[0]
    m = mc.master(H, k1, n2)
    alone = _run(H, k1, n2, m.x, m.g, 45)
    for n in (300,) + ((4097, 8200) if H in (32, 256) else ()):
        inside = _run(H, k1, n2, m.x, m.g, n)
        for k in mc.OUTPUTS:
            assert torch.equal(alone[k], inside[k][:45]), (H, n, k)
            assert torch.equal(inside[k][n - 8:], _run(H, k1, n2, m.x[n - 8:n], m.g[n - 8:n])[k]), (H, n, k, "last rows")


@pytest.mark.parametrize("k1,n2", [(128, 384), (256, 384), (352, 480)])
def test_hidden_128_is_the_128_wide_family(k1, n2):
    """xeq_mlp2h_* at hidden 128: the launch and the bits of xeq_mlp2_fwd / _bwd on the same packs, in the few-row and the 32-row form."""
    torch.manual_seed(k1)
    seq = torch.nn.Sequential(torch.nn.Linear(k1, 128), torch.nn.SiLU(), torch.nn.Linear(128, n2)).to(DEV).requires_grad_(False)
    pk = fused._mlp_packs(seq)
    small = int(lib.load().xeq_small_rows_limit())
    for n in (17, 300, small + 5):
        x, g = torch.randn(n, k1, device=DEV), torch.randn(n, n2, device=DEV)
        pre = [torch.empty(n, 128, device=DEV) for _ in range(2)]
        y = [torch.empty(n, n2, device=DEV) for _ in range(2)]
        gx = [torch.empty(n, k1, device=DEV) for _ in range(2)]
        first = lib.launch_count()
        call("xeq_mlp2_fwd", ptr(x), k1, n, k1, ptr(pk[0]), ptr(pk[1]), n2, ptr(pre[0]), ptr(y[0]), n2, stream())
        call("xeq_mlp2h_fwd", lib.XEQ_F32, ptr(x), k1, n, k1, 128, ptr(pk[0]), ptr(pk[1]), n2, ptr(pre[1]), ptr(y[1]), n2, stream())
        call("xeq_mlp2_bwd", ptr(g), n2, n, n2, ptr(pk[2]), ptr(pre[0]), ptr(pk[3]), k1, ptr(gx[0]), k1, stream())
        call("xeq_mlp2h_bwd", lib.XEQ_F32, ptr(g), n2, n, n2, 128, ptr(pk[2]), ptr(pre[0]), ptr(pk[3]), k1, ptr(gx[1]), k1, stream())
        assert lib.launch_names(first) == ["xeq_mlp2_fwd", "xeq_mlp2_fwd", "xeq_mlp2_bwd", "xeq_mlp2_bwd"]
        assert torch.equal(pre[0], pre[1]) and torch.equal(y[0], y[1]) and torch.equal(gx[0], gx[1]), n


def test_refusals_launch_nothing():
    w = torch.zeros(4096, device=DEV)
    p = ptr(w)
    for what, dtype, k1, H, n2 in mc.REFUSED:
        first = lib.launch_count()
        for name, args in (("xeq_mlp2h_fwd", (dtype, p, k1, 4, k1, H, p, p, n2, p, p, n2, stream())),
                           ("xeq_mlp2h_bwd", (dtype, p, k1, 4, k1, H, p, p, p, n2, p, n2, stream()))):
            assert getattr(lib.load(), name)(*args) == 1, (what, name)   # XEQ_ERR_INVALID_ARGUMENT
            msg = lib.load().xeq_last_error().decode()
            assert msg.startswith(name + ": needs f32, hidden % 32 == 0 in [32, 256], k1 % 32 == 0 and n2 % 32 == 0"), (what, msg)
            assert f"(got dtype {dtype}, k1 {k1}, hidden {H}, n2 {n2})" in msg, (what, msg)
            with pytest.raises(RuntimeError, match=name):
                call(name, *args)
        assert lib.launch_count() == first, what
    # inside the envelope: the row strides still have to fit
    with pytest.raises(RuntimeError, match="xeq_mlp2h_fwd: row strides"):
        call("xeq_mlp2h_fwd", lib.XEQ_F32, p, 34, 4, 32, 64, p, p, 32, p, p, 32, stream())
    with pytest.raises(RuntimeError, match="xeq_mlp2h_bwd: null buffer"):
        call("xeq_mlp2h_bwd", lib.XEQ_F32, p, 32, 4, 32, 64, p, None, p, 32, p, 32, stream())


def test_a_changed_bias_is_repacked():
    H, (k1, n2) = 64, mc.stacks(64)[0]
    seq = _seq(H, k1, n2)
    x = mc.master(H, k1, n2).x[:65].float().to(DEV)
    _, y0 = fused._mlp_fwd(seq, x)
    with torch.no_grad():
        seq[2].bias.add_(1.0)
    _, y1 = fused._mlp_fwd(seq, x)
    # the bias is the last term of the chain: y1 = fl(t + (b + 1)), y0 = fl(t + b) with |y| < 8: at most 3 roundings of 2^-22 apart
    assert float((y1 - y0 - 1.0).abs().max()) <= 3 * 2.0 ** -22 and float(y0.abs().max()) < 7.0
