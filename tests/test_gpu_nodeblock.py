"""Fused node-block kernels (csrc/xeq_nodeblock.hip) against the f64 oracle's restatement of XPainnUpdate.forward
(nn/xpainn.py:206-231) and the front half of XPainnMessage.forward (nn/xpainn.py:128-139), through the C ABI."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F_

pytestmark = pytest.mark.gpu

MUL = (128, 64, 32)
IRREPS = "128x0e + 64x1o + 32x2e"
F, C, D = 128, 224, 480


def _dev():
    return torch.device("cuda:0")


def _bt_to_mulir(buf, n, width):
    """BT buffer (width = 1: xhat-like, 2: the U|V pair buffer) -> list of mul_ir tensors [n, D] (one per column group)."""
    outs = [[] for _ in range(width)]
    base = 0
    for l, mul in enumerate(MUL):
        d = 2 * l + 1
        blk = buf[n * base * width: n * (base + d * mul) * width].view(n, d, width * mul)
        for k in range(width):
            outs[k].append(blk[:, :, k * mul:(k + 1) * mul].permute(0, 2, 1).reshape(n, mul * d))
        base += d * mul
    return [torch.cat(o, 1) for o in outs]


def _uv_native_to_mulir(buf, n):
    """The U|V buffer in the kernels' internal layout (tile numbering of csrc/xeq_nodeblock.hip::uv_tile) -> (U, V) in e3nn layout."""
    from xequinet_amd.nn import nodeblock

    rows = nodeblock.native_to_rows(buf, n, 2 * D).view(n, 2 * D // 32, 32)    # [n, tile, channel in tile]
    U, V = [], []
    tile = lambda l, m, v, c: 4 * v + c if l == 0 else (8 + 4 * m + 2 * v + c if l == 1 else 20 + 2 * m + v)
    for l, mul in enumerate(MUL):
        d = 2 * l + 1
        for v, out in ((0, U), (1, V)):
            blk = torch.stack([torch.cat([rows[:, tile(l, m, v, c)] for c in range(mul // 32)], 1) for m in range(d)], 2)   # [n, mul, d]
            out.append(blk.reshape(n, mul * d))
    return torch.cat(U, 1), torch.cat(V, 1)


def _close(name, got, ref, tol):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    assert err <= tol * scale, f"{name}: max abs err {err:.3e} (scale {scale:.3e}, tol {tol:.1e})"
    return err / scale


@pytest.mark.parametrize("form,n_ot", [(0, 4), (1, 4), (1, 7), (1, 18), (2, 4), (2, 18)])
@pytest.mark.parametrize("n", [1, 77, 128, 300])
def test_linear_primitives(form, n_ot, n):
    """Fragment maps, three-way split arithmetic and the weight ring: y = x W^T with asymmetric random operands."""
    from xequinet_amd.lib import call, ptr, stream

    torch.manual_seed(3 + n + n_ot)
    x = torch.randn(n, 128, device=_dev()) * torch.logspace(-3, 2, 128, device=_dev())[None, :]
    w = torch.randn(32 * n_ot, 128, device=_dev())
    scratch = torch.empty(8 * n_ot * 3072 + 4 * 3072, dtype=torch.uint8, device=_dev())
    y = torch.full((n, 32 * n_ot), float("nan"), device=_dev())
    call("xeq_node_block_linear_test", ptr(x), n, ptr(w), n_ot, form, ptr(scratch), ptr(y), stream())
    torch.cuda.synchronize()
    ref = x.double() @ w.double().t()
    mag = x.double().abs() @ w.double().abs().t()      # the bound is relative to sum |x| |w| (f32 accumulation)
    err = ((y.double() - ref).abs() / mag).max().item()
    assert err <= 3e-7, err


def _modules(seed):
    from xequinet_amd.nn.xpainn import XPainnMessage, XPainnUpdate

    torch.manual_seed(seed)
    upd = XPainnUpdate(node_dim=F, node_irreps=IRREPS)
    msg = XPainnMessage(node_dim=F, node_irreps=IRREPS)
    with torch.no_grad():   # non-trivial affine parameters and biases
        for mod in (upd, msg):
            mod.norm.weight.uniform_(0.5, 1.5)
            mod.norm.bias.normal_(0, 0.3)
            mod.o3norm.affine_weight.uniform_(0.5, 1.5)
            mod.o3norm.affine_bias.normal_(0, 0.3)
        upd.update_U.bias.normal_(0, 0.3)
        upd.update_V.bias.normal_(0, 0.3)
    return upd, msg


def _reference(upd, msg, s, x, dtype=torch.float64):
    """f64 restatement with the oracle's operator definitions (``dtype``: the same restatement in another precision, on the CPU)."""
    from oracle import xpainn_oracle as orc

    sd = {k: v.detach().to(dtype).cpu() for k, v in upd.state_dict().items()}
    s, x = s.to(dtype).cpu(), x.to(dtype).cpu()
    n = s.shape[0]
    out = {}
    mean = s.mean(1)
    var = s.var(1, unbiased=False)
    x0 = x[:, :MUL[0]]
    mean0 = x0.mean(1)
    xc = x.clone()
    xc[:, :MUL[0]] -= mean0[:, None]
    sq = torch.zeros(n, dtype=dtype)
    off = 0
    for l, mul in enumerate(MUL):
        d = 2 * l + 1
        sq += (xc[:, off:off + mul * d] ** 2).sum(1)
        off += mul * d
    rr = 1.0 / torch.sqrt(sq / C + 1e-5)
    out["stats"] = torch.stack([mean, 1.0 / torch.sqrt(var + 1e-5), mean0, rr], 1)
    shat = F_.layer_norm(s, (F,), sd["norm.weight"], sd["norm.bias"], 1e-5)
    xhat = orc.equivariant_layer_norm(IRREPS, x, sd["o3norm.affine_weight"], sd["o3norm.affine_bias"])
    U = orc.o3_linear(IRREPS, xhat, sd["update_U.weight"], sd["update_U.bias"])
    V = orc.o3_linear(IRREPS, xhat, sd["update_V.weight"], sd["update_V.bias"])
    out["U"], out["V"] = U, V
    v = orc.invariant(IRREPS, V, eps=upd.invariant.eps)
    pre = F_.linear(torch.cat([shat, v], -1), sd["update_mlp.0.weight"], sd["update_mlp.0.bias"])
    out["pre"] = pre
    a = F_.linear(F_.silu(pre), sd["update_mlp.2.weight"], sd["update_mlp.2.bias"])
    out["a"] = a
    a_vv, a_sv, a_ss = torch.split(a, [C, F, F], dim=-1)
    ip = F_.linear(orc.equivariant_dot(IRREPS, U, V), sd["dot_lin.weight"])
    out["ip"] = ip
    s2 = s + a_sv * ip + a_ss
    x2 = x + orc.elementwise_tp(IRREPS, U, a_vv)
    out["s_out"], out["x_out"] = s2, x2
    if msg is not None:
        md = {k: v.detach().to(dtype).cpu() for k, v in msg.state_dict().items()}
        shat2 = F_.layer_norm(s2, (F,), md["norm.weight"], md["norm.bias"], 1e-5)
        out["xhat2"] = orc.equivariant_layer_norm(IRREPS, x2, md["o3norm.affine_weight"], md["o3norm.affine_bias"])
        pre2 = F_.linear(shat2, md["scalar_mlp.0.weight"], md["scalar_mlp.0.bias"])
        out["pre2"] = pre2
        out["h2"] = F_.linear(F_.silu(pre2), md["scalar_mlp.2.weight"], md["scalar_mlp.2.bias"])
        x20 = x2[:, :MUL[0]]
        m20 = x20.mean(1)
        xc2 = x2.clone()
        xc2[:, :MUL[0]] -= m20[:, None]
        out["stats2"] = torch.stack([s2.mean(1), 1.0 / torch.sqrt(s2.var(1, unbiased=False) + 1e-5), m20,
                                     1.0 / torch.sqrt((xc2 ** 2).sum(1) / C + 1e-5)], 1)
    return out


@pytest.mark.parametrize("n", [5, 128, 333])
@pytest.mark.parametrize("tail", [True, False])
def test_node_block_forward_matches_f64(n, tail):
    from xequinet_amd.nn import nodeblock

    upd, msg = _modules(11)
    upd, msg = upd.to(_dev()), msg.to(_dev())
    assert nodeblock.supported(upd, msg)
    torch.manual_seed(100 + n)
    s = torch.randn(n, F, device=_dev()) * 1.5 + 0.2
    x = torch.randn(n, D, device=_dev()) * 0.8
    got = nodeblock.node_block_fwd(s, x, upd, msg if tail else None, want_x=True)
    torch.cuda.synchronize()
    ref = _reference(upd, msg if tail else None, s, x)
    U, V = _uv_native_to_mulir(got["uv"], n)
    for k, width in (("pre", F), ("a", C + 2 * F), ("ip", F)) + ((("pre2", F),) if tail else ()):
        got[k] = nodeblock.native_to_rows(got[k], n, width)
    tol = 3e-6
    worst = {}
    worst["U"] = _close("U", U, ref["U"], tol)
    worst["V"] = _close("V", V, ref["V"], tol)
    for k in ("stats", "pre", "a", "ip", "s_out", "x_out"):
        worst[k] = _close(k, got[k], ref[k], tol)
    if tail:
        (xhat2,) = _bt_to_mulir(got["xhat2"], n, 1)
        worst["xhat2"] = _close("xhat2", xhat2, ref["xhat2"], tol)
        for k in ("stats2", "pre2", "h2"):
            worst[k] = _close(k, got[k], ref[k], tol)
    print("relative errors:", {k: f"{v:.1e}" for k, v in worst.items()})


def test_node_block_forward_rows_do_not_depend_on_the_batch():
    """A node's bits are the same whatever rows share its wave (sharded / chunked / padded batches agree bit for bit)."""
    from xequinet_amd.nn import nodeblock

    upd, msg = _modules(12)
    upd, msg = upd.to(_dev()), msg.to(_dev())
    torch.manual_seed(5)
    s = torch.randn(300, F, device=_dev())
    x = torch.randn(300, D, device=_dev())
    full = nodeblock.node_block_fwd(s, x, upd, msg)
    part = nodeblock.node_block_fwd(s[37:171].contiguous(), x[37:171].contiguous(), upd, msg)
    torch.cuda.synchronize()
    for k in ("s_out", "x_out", "h2"):
        assert torch.equal(full[k][37:171], part[k]), k
    for k, width in (("pre2", F), ("a", C + 2 * F), ("ip", F), ("pre", F)):
        assert torch.equal(nodeblock.native_to_rows(full[k], 300, width)[37:171], nodeblock.native_to_rows(part[k], 134, width)), k


def _reference_diff(upd, msg, s, x, dtype=torch.float64):
    """The same restatement as a differentiable f64 function of (s, x) -> (s_out, x_out[, h2, xhat2 (e3nn layout)]);
    ``dtype``: the precision of the weights (s, x are taken as given)."""
    from oracle import xpainn_oracle as orc

    sd = {k: v.detach().to(dtype).cpu() for k, v in upd.state_dict().items()}
    shat = F_.layer_norm(s, (F,), sd["norm.weight"], sd["norm.bias"], 1e-5)
    xhat = orc.equivariant_layer_norm(IRREPS, x, sd["o3norm.affine_weight"], sd["o3norm.affine_bias"])
    U = orc.o3_linear(IRREPS, xhat, sd["update_U.weight"], sd["update_U.bias"])
    V = orc.o3_linear(IRREPS, xhat, sd["update_V.weight"], sd["update_V.bias"])
    v = orc.invariant(IRREPS, V, eps=upd.invariant.eps)
    a = F_.linear(F_.silu(F_.linear(torch.cat([shat, v], -1), sd["update_mlp.0.weight"], sd["update_mlp.0.bias"])),
                  sd["update_mlp.2.weight"], sd["update_mlp.2.bias"])
    a_vv, a_sv, a_ss = torch.split(a, [C, F, F], dim=-1)
    ip = F_.linear(orc.equivariant_dot(IRREPS, U, V), sd["dot_lin.weight"])
    s2 = s + a_sv * ip + a_ss
    x2 = x + orc.elementwise_tp(IRREPS, U, a_vv)
    if msg is None:
        return s2, x2
    md = {k: v.detach().to(dtype).cpu() for k, v in msg.state_dict().items()}
    shat2 = F_.layer_norm(s2, (F,), md["norm.weight"], md["norm.bias"], 1e-5)
    xhat2 = orc.equivariant_layer_norm(IRREPS, x2, md["o3norm.affine_weight"], md["o3norm.affine_bias"])
    h2 = F_.linear(F_.silu(F_.linear(shat2, md["scalar_mlp.0.weight"], md["scalar_mlp.0.bias"])), md["scalar_mlp.2.weight"],
                   md["scalar_mlp.2.bias"])
    return s2, x2, h2, xhat2


def _mulir_to_bt(t):
    """[n, D] e3nn layout -> flat BT buffer"""
    n = t.shape[0]
    parts, off = [], 0
    for l, mul in enumerate(MUL):
        d = 2 * l + 1
        parts.append(t[:, off:off + mul * d].reshape(n, mul, d).permute(0, 2, 1).reshape(-1))
        off += mul * d
    return torch.cat(parts)


@pytest.mark.parametrize("n", [5, 128, 333])
@pytest.mark.parametrize("mode", ["tail", "gx", "last"])
def test_node_block_backward_matches_f64_autograd(n, mode):
    from xequinet_amd.nn import nodeblock

    upd, msg = _modules(21)
    upd, msg = upd.to(_dev()), msg.to(_dev())
    tail = mode == "tail"
    torch.manual_seed(200 + n)
    s = torch.randn(n, F, device=_dev()) * 1.5 + 0.2
    x = torch.randn(n, D, device=_dev()) * 0.8
    saved = nodeblock.node_block_fwd(s, x, upd, msg if tail else None, want_x=True)
    g_s_in = torch.randn(n, F, device=_dev())
    g_x_in = torch.randn(n, D, device=_dev()) if mode != "last" else None
    g_h = torch.randn(n, F + 2 * C, device=_dev()) if tail else None
    g_xh = torch.randn(n, D, device=_dev()) if tail else None        # e3nn layout; handed over in BT
    g_s, g_x = nodeblock.node_block_bwd(saved, s, x, upd, msg if tail else None, g_s_in, g_x_in,
                                        g_h, _mulir_to_bt(g_xh) if tail else None)
    torch.cuda.synchronize()
    sd_, xd_ = s.double().cpu().requires_grad_(), x.double().cpu().requires_grad_()
    outs = _reference_diff(upd, msg if tail else None, sd_, xd_)
    cot = [g_s_in.double().cpu(), g_x_in.double().cpu() if g_x_in is not None else torch.zeros(n, D, dtype=torch.float64)]
    if tail:
        cot += [g_h.double().cpu(), g_xh.double().cpu()]
    ref_s, ref_x = torch.autograd.grad(outs, (sd_, xd_), cot)
    e1 = _close("g_s", g_s, ref_s, 2e-5)   # f32 chain; 1 / |V| of the invariant conditions the tail
    e2 = _close("g_x", g_x, ref_x, 2e-5)
    print(f"relative errors: g_s {e1:.1e}, g_x {e2:.1e}")


def test_node_block_at_full_size_equals_itself_on_slices():
    """86 016 nodes (the MD17 x 4096 batch: several rounds of workgroups per CU, two workgroups resident per CU) against the same
    launches on slices of a few hundred rows, BIT FOR BIT, forward and reverse: a node's result may not depend on how full the chip is.
    (The 16-node form of these kernels passed every small-size test and failed exactly this while it was compiled with packed-fp32
    instructions -- sporadic wrong values in one 16-lane row once two waves shared a SIMD, profiles/r04_nodeblock.txt item 9 -- so
    the property is pinned at a size where it can break.)"""
    from xequinet_amd.nn import nodeblock

    n = 86016
    upd, msg = _modules(3)
    upd, msg = upd.to(_dev()), msg.to(_dev())
    torch.manual_seed(1)
    s = torch.randn(n, F, device=_dev())
    x = torch.randn(n, D, device=_dev())
    g_s_in, g_x_in = torch.randn(n, F, device=_dev()), torch.randn(n, D, device=_dev())
    g_h, g_xh = torch.randn(n, F + 2 * C, device=_dev()), torch.randn(n, D, device=_dev())
    for rep in range(2):
        full = nodeblock.node_block_fwd(s, x, upd, msg, want_x=True)
        g_s, g_x = nodeblock.node_block_bwd(full, s, x, upd, msg, g_s_in, g_x_in, g_h, _mulir_to_bt(g_xh))
        torch.cuda.synchronize()
        for a in range(0, n, 3072):
            b = min(n, a + 300)
            sp, xp = s[a:b].contiguous(), x[a:b].contiguous()
            part = nodeblock.node_block_fwd(sp, xp, upd, msg, want_x=True)
            for k in ("s_out", "x_out", "h2"):
                assert torch.equal(full[k][a:b], part[k]), (rep, a, k)
            for k, width in (("pre2", F), ("a", C + 2 * F), ("ip", F), ("pre", F)):
                assert torch.equal(nodeblock.native_to_rows(full[k], n, width)[a:b], nodeblock.native_to_rows(part[k], b - a, width)), (rep, a, k)
            gs2, gx2 = nodeblock.node_block_bwd(part, sp, xp, upd, msg, g_s_in[a:b].contiguous(), g_x_in[a:b].contiguous(), g_h[a:b].contiguous(),
                                                _mulir_to_bt(g_xh[a:b].contiguous()))
            assert torch.equal(g_s[a:b], gs2) and torch.equal(g_x[a:b], gx2), (rep, a)


@pytest.mark.parametrize("n", [18609, 24000, 32768])
def test_node_block_results_do_not_depend_on_the_waves_per_workgroup(n, monkeypatch):
    """Between one and two four-wave workgroups per CU a launch takes one workgroup of 5 .. 8 waves per CU (xeq::nb::waves_for, round 5:
    no CU with twice the load of another).  A wave's 16 nodes see the same weights in the same order in any workgroup: forward and
    reverse results with the automatic choice equal those of four-wave and of eight-wave workgroups BIT FOR BIT, and repeat."""
    from xequinet_amd.nn import nodeblock

    upd, msg = _modules(3)
    upd, msg = upd.to(_dev()), msg.to(_dev())
    torch.manual_seed(2)
    s = torch.randn(n, F, device=_dev())
    x = torch.randn(n, D, device=_dev())
    g_s_in, g_x_in = torch.randn(n, F, device=_dev()), torch.randn(n, D, device=_dev())
    g_h, g_xh = torch.randn(n, F + 2 * C, device=_dev()), _mulir_to_bt(torch.randn(n, D, device=_dev()))

    def run():
        full = nodeblock.node_block_fwd(s, x, upd, msg, want_x=True)
        g = nodeblock.node_block_bwd(full, s, x, upd, msg, g_s_in, g_x_in, g_h, g_xh)
        return [full[k].clone() for k in ("s_out", "x_out", "h2", "xhat2")] + [t.clone() for t in g]

    monkeypatch.delenv("XEQ_NODE_BLOCK_WAVES", raising=False)
    auto = run()
    again = run()
    outs = {}
    for w in ("4", "8"):
        monkeypatch.setenv("XEQ_NODE_BLOCK_WAVES", w)
        outs[w] = run()
    monkeypatch.delenv("XEQ_NODE_BLOCK_WAVES")
    for other in (again, outs["4"], outs["8"]):
        for a, b in zip(auto, other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("how", ["in_place", "new_storage"])
def test_packs_follow_every_weight_that_feeds_them(how):
    """No packed copy outlives a change of a weight it was made from: after every single change -- in place (the version counter moves)
    or as a new storage under the same parameter (the address moves) -- an update block + next message block pair gives, bit for bit,
    what a freshly constructed pair holding the same weights gives.  Both the fused node block and the update block's own kernels."""
    from xequinet_amd.nn import fused

    dev = _dev()
    n = 4100
    upd, msg = (m.to(dev).eval().requires_grad_(False) for m in _modules(5))
    D = upd.node_irreps.dim
    g = torch.Generator().manual_seed(0)
    s0, x0 = torch.randn(n, F, generator=g).to(dev), torch.randn(n, D, generator=g).to(dev)
    g_out = [torch.randn(*shape, generator=g).to(dev) for shape in ((n, F), (n, D), (n, msg.hidden_dim), (n * D,))]

    def evaluate(u, m):
        s, x = s0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        with torch.enable_grad():
            block = fused.NodeBlock.apply(s, x, u, m)
            g_block = torch.autograd.grad(block, [s, x], g_out)
            chain = fused.UpdateBlock.apply(s, x, u)
            g_chain = torch.autograd.grad(chain, [s, x], g_out[:2])
        return [t.detach() for t in (*block, *g_block, *chain, *g_chain)]

    evaluate(upd, msg)
    weights = {"update_mlp.0.weight": upd.update_mlp[0].weight, "update_mlp.0.bias": upd.update_mlp[0].bias,
               "update_mlp.2.weight": upd.update_mlp[2].weight, "update_mlp.2.bias": upd.update_mlp[2].bias,
               "update_U.weight": upd.update_U.weight, "update_U.bias": upd.update_U.bias, "update_V.weight": upd.update_V.weight,
               "update_V.bias": upd.update_V.bias, "dot_lin.weight": upd.dot_lin.weight, "next scalar_mlp.0.weight": msg.scalar_mlp[0].weight,
               "next scalar_mlp.0.bias": msg.scalar_mlp[0].bias, "next scalar_mlp.2.weight": msg.scalar_mlp[2].weight,
               "next scalar_mlp.2.bias": msg.scalar_mlp[2].bias}
    for name, p in weights.items():
        with torch.no_grad():
            if how == "in_place":
                p.mul_(1.25).add_(0.01)
            else:
                p.data = p.data * 1.25 + 0.01
        fresh_u, fresh_m = (m.to(dev).eval().requires_grad_(False) for m in _modules(6))
        fresh_u.load_state_dict(upd.state_dict())
        fresh_m.load_state_dict(msg.state_dict())
        for k, (got, want) in enumerate(zip(evaluate(upd, msg), evaluate(fresh_u, fresh_m))):
            assert torch.equal(got, want), f"after a change of {name} ({how}): output {k} differs by {(got - want).abs().max().item():.2e}"
