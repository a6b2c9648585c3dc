"""The node kernels of the twice-differentiable training pass alone (csrc/xeq_train_node.hip: xeq_train_norm, xeq_train_uv, xeq_train_out;
nn/training_ops.py), each in its four forms -- forward, reverse, forward with tangents, reverse with tangents -- in f32 and f64, against
``three_orders`` of the plain-tensor restatement in f64 (tests/train_node_cases.py), at the widths and row counts of real models: lane
loops with a partial last round, C < F, every mul[l] == 0, both xhat layouts, row counts on both sides of a four-wave block and of a
256-thread block, and 16 389 rows, where the grid-stride loop of the norm kernels makes a second round.

Entry level: every input sits between guard bands, every output is a ``torch.empty`` of training_ops taken from
``guard_allocations()``, so it is handed over holding the never-written pattern between bands of its own (tests/guard_bands.py).

Bounds, per output and row group (ordinary rows, the all-zero row, the row scaled by 1e3, in f64 the rows with V_0 near zero); the
figures and the rule are those of tests/test_gpu_train_edge.py:
  f64  values 1e-12, derivatives of both orders 1e-9, of the largest entry of the output in the group, at least the ordinary group's;
  f32  max(4 x the f32 restatement's own error against f64 on the same inputs, 4 ulp of that largest entry).
tests/test_train_node_cases_host.py shows that every defect of its list leaves these bounds.  Every figure is printed before it is
asserted (``train-node ...`` lines: profiles/train_node_parity.txt is their summary)."""
import pytest
import torch

from tests import guard_bands as gb, train_node_cases as tc
from tests.update_cases import dims, to_bt
from xequinet_amd import lib
from xequinet_amd.nn import training_ops as to

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = {"f32": torch.float32, "f64": torch.float64}
CONFIG_IDS = [tc.config_id(*c) for c in tc.CONFIGS]


def _in(t, dtype):
    return gb.guarded_copy(t.to(dtype).to(DEV).contiguous())


def _written(outs, net):
    """The bands were checked when the block ended; here: every output came from the net and holds no never-written word."""
    assert net.count == len(outs), (net.count, len(outs))
    for t in outs:
        assert gb.guard_of(t) in net.records
        assert not bool(gb.unwritten(t).any()), ("unwritten", tuple(t.shape), int(gb.unwritten(t).sum()))


def _split_rows(rows, F, C):
    return [rows[:, :F], rows[:, F:2 * F], rows[:, 2 * F:2 * F + C], rows[:, 2 * F + C:]]


def _run(kind, c, dtype):
    """The four forms of the entry on the case -> name -> [n, .] rows on the CPU."""
    F, mul, n = c.F, c.mul, c.n
    D, C = dims(mul)
    t = lambda v: _in(v, dtype)
    cpu = lambda ts: [v.cpu() for v in ts]
    if kind in ("norm0", "norm1"):
        layout = int(kind == "norm1")
        meta = (F, mul, tc.EPS_LN, tc.EPS_EQ, layout)
        s, x, u_s, u_x, g_s = (t(getattr(c, k)) for k in ("s", "x", "u_s", "u_x", "g_s"))
        g_x = t(to_bt(c.g_x, mul) if layout else c.g_x)
        prm = [t(getattr(c, k)) for k in tc.PARAMS]        # (mul[0] == 0: eq_b is empty; its pointer is the band's, the kernel never reads it)
        ins = [s, x, u_s, u_x, g_s, g_x, *prm]
        with gb.guard_allocations() as net:
            f_s, f_x, none = to._norm_call(0, s, None, x, None, *prm, None, None, meta)
            b_s, b_x, b_rows = to._norm_call(1, s, None, x, None, *prm, g_s, g_x, meta)
            fd_s, fd_x, _ = to._norm_call(0, s, u_s, x, u_x, *prm, None, None, meta)
            bd_s, bd_x, bd_rows = to._norm_call(1, s, u_s, x, u_x, *prm, g_s, g_x, meta)
        assert none is None and f_x.shape == ((n * D,) if layout else (n, D)) and b_x.shape == (n, D) and b_rows.shape == (n, 2 * F + C + mul[0])
        _written([f_s, f_x, b_s, b_x, b_rows, fd_s, fd_x, bd_s, bd_x, bd_rows], net)
        # the cotangent carries no tangent: d ln_b and d eq_b of the dual reverse form are exact zeros
        assert not bool(bd_rows[:, F:2 * F].any()) and not bool(bd_rows[:, 2 * F + C:].any())
        forms = (cpu([f_s, f_x]), cpu([b_s, b_x, *_split_rows(b_rows, F, C)]), cpu([fd_s, fd_x]), cpu([bd_s, bd_x, *_split_rows(bd_rows, F, C)]))
    else:
        uv, u_uv = [t(v) for v in tc.uv_list(c.U, c.V, mul)], [t(v) for v in tc.uv_list(c.u_U, c.u_V, mul)]
        if kind == "uv":
            meta = (mul, tc.EPS_INV)
            g = t(c.g_vd)
            ins = [*uv, *u_uv, g]
            with gb.guard_allocations() as net:
                o = to._uv_call(0, uv, None, None, meta)
                d_uv = to._uv_call(1, uv, None, g, meta)
                dg = to._uv_call(0, uv, u_uv, None, meta)
                dd_uv = to._uv_call(1, uv, u_uv, g, meta)
            assert o.shape == (n, 2 * C)
            _written([o, *d_uv, dg, *dd_uv], net)
            forms = (cpu([o]), cpu(d_uv), cpu([dg]), cpu(dd_uv))
        else:
            meta = (F, mul)
            a, inner, u_a, u_in, g_s, g_x = (t(getattr(c, k)) for k in ("a", "inner", "u_a", "u_in", "g_os", "g_ox"))
            ins = [*uv, *u_uv, a, inner, u_a, u_in, g_s, g_x]
            with gb.guard_allocations() as net:
                o_s, o_x = to._out_call(0, uv, None, a, None, inner, None, None, None, meta)
                d_uv, d_a, d_in = to._out_call(1, uv, None, a, None, inner, None, g_s, g_x, meta)
                dg_s, dg_x = to._out_call(0, uv, u_uv, a, u_a, inner, u_in, None, None, meta)
                dd_uv, dd_a, dd_in = to._out_call(1, uv, u_uv, a, u_a, inner, u_in, g_s, g_x, meta)
            assert o_s.shape == (n, F) and o_x.shape == (n, D)
            _written([o_s, o_x, *d_uv, d_a, d_in, dg_s, dg_x, *dd_uv, dd_a, dd_in], net)
            forms = (cpu([o_s, o_x]), cpu([*d_uv, d_a, d_in]), cpu([dg_s, dg_x]), cpu([*dd_uv, dd_a, dd_in]))
    gb.check(*ins)
    got = tc.as_rows(kind, forms, n, mul)
    if kind == "out":          # nothing depends on V: its half of d_uv is written, with exact zeros, in the plain and the dual form
        assert not bool(got["d_uv"][:, tc.v_half(mul)].any()) and not bool(got["dd_uv"][:, tc.v_half(mul)].any())
    return got


class _Record:
    """Every figure of one test, printed as it comes; the worst per (kind, form, output) printed and the failures asserted at the end."""

    def __init__(self, tag, f64, level="entry"):
        self.tag, self.f64, self.level, self.worst, self.failed = tag, f64, level, {}, []

    def add(self, kind, res, what):
        form_of = {k: form for form, names in tc.FORMS[kind].items() for k in names} if kind in tc.FORMS else {}      # (the sums: no form)
        for k, grp, err, chain, bnd in res:
            ratio = err / bnd if bnd > 0 else (0.0 if err == 0 else float("inf"))
            print(f"train-node {self.tag} {kind} {what} {k} {grp}: kernel {err:.3e} chain {chain:.3e} kernel/chain {err / max(chain, 1e-300):.2f} "
                  f"bound {bnd:.3e} kernel/bound {ratio:.3f}")
            key = (kind, form_of.get(k, "bwd"), k)
            if ratio > self.worst.get(key, (-1.0,))[0]:
                self.worst[key] = (ratio, err, chain, bnd, f"{what} {grp}")
            if not err <= bnd:
                self.failed.append((kind, what, k, grp, err, chain, bnd))

    def close(self):
        for (kind, form, k), (ratio, err, chain, bnd, what) in sorted(self.worst.items()):
            print(f"train-node-worst {self.level} {'f64' if self.f64 else 'f32'} {kind} {form} {k}: kernel/bound {ratio:.3f} kernel {err:.3e} chain {chain:.3e} "
                  f"bound {bnd:.3e} ({self.tag} {what})")
        assert not self.failed, (self.tag, self.failed)


# ---------------------------------------------------------------------------------------------------------------------- entry level
_SHORT = {}      # (kind, precision) -> rows of the 257-row run at tc.LONG, for the row-independence test


@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("F,mul", tc.CONFIGS, ids=CONFIG_IDS)
def test_entries_against_the_f64_restatement(F, mul, prec):
    """Every entry in its four forms at every row count; in f64 on the variant of the draw that holds the near-zero V_0 rows."""
    f64 = prec == "f64"
    rec = _Record(f"{tc.config_id(F, mul)} {prec}", f64)
    for kind in tc.KINDS:
        for n in tc.ROWS:
            c = tc.case(kind, F, mul, n, near=f64)
            got = _run(kind, c, PRECISIONS[prec])
            rec.add(kind, tc.judge(c.ref, c.ref32, got, tc.outputs(kind), n, f64, near=f64), f"n={n}")
    rec.close()


def _long(kind, prec):
    """The 16 389-row run of ``kind``: judged once, its first 257 rows kept."""
    key = (kind, prec)
    if key not in _LONG:
        F, mul = tc.LONG
        c = tc.case(kind, F, mul, tc.LONG_ROWS)
        got = _run(kind, c, PRECISIONS[prec])
        res = tc.judge(c.ref, c.ref32, got, tc.outputs(kind), tc.LONG_ROWS, prec == "f64")
        _LONG[key] = (res, {k: v[:tc.ROWS_MASTER].clone() for k, v in got.items()})
    return _LONG[key]


_LONG = {}


@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("kind", tc.KINDS)
def test_second_grid_stride_round(kind, prec):
    """16 389 rows of 152 floats: the norm kernels' grid of 4096 blocks of four waves makes a second round with a partial last block."""
    assert tc.LONG_ROWS > 4 * 4096
    rec = _Record(f"{tc.config_id(*tc.LONG)} {prec}", prec == "f64")
    rec.add(kind, _long(kind, prec)[0], f"n={tc.LONG_ROWS}")
    rec.close()


@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("kind", tc.KINDS)
def test_a_row_does_not_depend_on_the_rows_around_it(kind, prec):
    """Rows 0 .. 256 of the 16 389-row run have the bits of the 257-row run, in every form (the BT layout compared row by row)."""
    F, mul = tc.LONG
    short = _run(kind, tc.case(kind, F, mul, tc.ROWS_MASTER), PRECISIONS[prec])
    long = _long(kind, prec)[1]
    for k in tc.outputs(kind):
        assert torch.equal(short[k], long[k]), (kind, prec, k, float((short[k] - long[k]).abs().max()))


# ------------------------------------------------------------------------------------------------------------- through the Functions
def _whole(v):
    return v.reshape(1, -1)


def _function_forms(kind, c, dtype, on_gpu):
    """three_orders of the Function (``on_gpu``) or of the restatement, parameters shared by the rows -> (rows: name -> [n, .],
    sums: name -> [1, .])."""
    F, mul, n = c.F, c.mul, c.n
    D, C = dims(mul)
    t = (lambda v: v.detach().to(dtype).to(DEV)) if on_gpu else (lambda v: v.detach().to(dtype))
    back = lambda v: v.detach().cpu()
    if kind in ("norm0", "norm1"):
        layout = int(kind == "norm1")
        meta = (F, mul, tc.EPS_LN, tc.EPS_EQ, layout)
        if on_gpu:
            fn = lambda *a: to.NormFn.apply(*a, meta)
        else:
            def fn(*a):
                o_s, o_x = tc.norm(*a, F, mul, tc.EPS_LN, tc.EPS_EQ)
                return o_s, (to_bt(o_x, mul) if layout else o_x)
        inputs = [t(c.s), t(c.x)] + [t(getattr(c, k)) for k in tc.PARAMS]
        g = [t(c.g_s), t(to_bt(c.g_x, mul) if layout else c.g_x)]
        vals, first, d_g, d_in = tc.three_orders(fn, inputs, g, [t(c.u_s), t(c.u_x), None, None, None, None])
        vals, first, d_g, d_in = ([back(v) for v in part] for part in (vals, first, d_g, d_in))
        x_rows = (lambda v: tc.from_bt(v, n, mul)) if layout else (lambda v: v)
        rows = {"o_s": vals[0], "o_x": x_rows(vals[1]), "d_s": first[0], "d_x": first[1], "dg_s": d_g[0], "dg_x": x_rows(d_g[1]),
                "dd_s": d_in[0], "dd_x": d_in[1]}
        sums = {"d_ln_w": first[2], "d_ln_b": first[3], "d_eq_w": first[4], "dd_ln_w": d_in[2], "dd_eq_w": d_in[4]}
        if mul[0]:
            sums["d_eq_b"] = first[5]
        return rows, {k: _whole(v) for k, v in sums.items()}
    spec = tc.call_spec(kind, c, dtype)
    if on_gpu:
        fn = (lambda a, b, d: to.UvFn.apply(a, b, d, (mul, tc.EPS_INV))) if kind == "uv" else (lambda *a: to.UpdateOutFn.apply(*a, (F, mul)))
        spec = (fn, *[[None if v is None else v.to(DEV) for v in part] for part in spec[1:]])
    forms = [[back(v) for v in part] for part in tc.three_orders(*spec)]
    return tc.as_rows(kind, forms, n, mul), {}


@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("F,mul", tc.FUNCTION_CONFIGS, ids=[tc.config_id(*c) for c in tc.FUNCTION_CONFIGS])
def test_functions_in_three_orders(F, mul, prec):
    """NormFn (both layouts), UvFn and UpdateOutFn through autograd: values, the first order -- the parameter gradients of the norm, summed
    over the rows, among them -- and the second order with respect to cotangents, inputs and ln_w, eq_w; the same bounds, the sums judged
    as one group each."""
    f64, n = prec == "f64", tc.ROWS_MASTER
    c = tc.take(tc.master(F, mul), n)
    rec = _Record(f"{tc.config_id(F, mul)} {prec} functions", f64, "function")
    for kind in tc.KINDS:
        ref, ref_sums = _function_forms(kind, c, torch.float64, False)
        ref32, ref32_sums = _function_forms(kind, c, torch.float32, False)
        first = lib.launch_count()
        with gb.guard_allocations():
            got, got_sums = _function_forms(kind, c, PRECISIONS[prec], True)
        assert {"norm0": "xeq_train_norm", "norm1": "xeq_train_norm", "uv": "xeq_train_uv", "out": "xeq_train_out"}[kind] in lib.launch_names(first)
        assert set(got) == set(ref) and set(got_sums) == set(ref_sums)
        rec.add(kind, tc.judge(ref, ref32, got, sorted(ref), n, f64), f"n={n}")
        if ref_sums:
            rec.add(kind + "-sums", tc.judge(ref_sums, ref32_sums, got_sums, sorted(ref_sums), 1, f64), f"n={n}")
    rec.close()


# --------------------------------------------------------------------------------------------------------------- refusals and empties
def _small(dtype=torch.float64, n=3):
    F, mul = 6, (5, 3, 2)
    c = tc.take(tc.master(F, mul), n)
    t = lambda v: v.to(dtype).to(DEV).contiguous()
    return c, t


def test_entries_refuse_what_they_cannot_run_and_launch_nothing():
    """The reverse form without (one of) its cotangents, one tangent of a pair without the other, layout 2, no channels: the entry's own
    error through lib.call, nothing launched."""
    c, t = _small()
    F, mul = c.F, c.mul
    s, x, u_s, u_x, g_s, g_x = (t(getattr(c, k)) for k in ("s", "x", "u_s", "u_x", "g_s", "g_x"))
    prm = [t(getattr(c, k)) for k in tc.PARAMS]
    uv, u_uv = [t(v) for v in tc.uv_list(c.U, c.V, mul)], [t(v) for v in tc.uv_list(c.u_U, c.u_V, mul)]
    a, inner, u_a, u_in, g_os, g_ox, g_vd = (t(getattr(c, k)) for k in ("a", "inner", "u_a", "u_in", "g_os", "g_ox", "g_vd"))
    norm_meta = (F, mul, tc.EPS_LN, tc.EPS_EQ, 0)
    empty = [s.new_zeros(0)] * 3
    first = lib.launch_count()
    refused = [
        ("xeq_train_norm: the reverse form needs", lambda: to._norm_call(1, s, None, x, None, *prm, None, None, norm_meta)),
        ("xeq_train_norm: the reverse form needs", lambda: to._norm_call(1, s, None, x, None, *prm, g_s, None, norm_meta)),
        ("xeq_train_uv: the reverse form needs g", lambda: to._uv_call(1, uv, None, None, (mul, tc.EPS_INV))),
        ("xeq_train_out: the reverse form needs", lambda: to._out_call(1, uv, None, a, None, inner, None, None, None, (F, mul))),
        ("xeq_train_out: the reverse form needs", lambda: to._out_call(1, uv, None, a, None, inner, None, g_os, None, (F, mul))),
        ("xeq_train_norm: tangents of s and x come together", lambda: to._norm_call(0, s, u_s, x, None, *prm, None, None, norm_meta)),
        ("xeq_train_norm: tangents of s and x come together", lambda: to._norm_call(1, s, None, x, u_x, *prm, g_s, g_x, norm_meta)),
        ("xeq_train_out: the tangents come together", lambda: to._out_call(0, uv, u_uv, a, None, inner, u_in, None, None, (F, mul))),
        ("xeq_train_out: the tangents come together", lambda: to._out_call(0, uv, None, a, u_a, inner, None, None, None, (F, mul))),
        ("xeq_train_norm: layout 2", lambda: to._norm_call(0, s, None, x, None, *prm, None, None, (F, mul, tc.EPS_LN, tc.EPS_EQ, 2))),
        ("xeq_train_norm: no channels", lambda: to._norm_call(0, s, None, x[:, :0].contiguous(), None, prm[0], prm[1], empty[0], empty[0], None, None,
                                                              (F, (0, 0, 0), tc.EPS_LN, tc.EPS_EQ, 0))),
        ("xeq_train_uv: no channels", lambda: lib.call("xeq_train_uv", lib.dtype_code(s), 0, c.n, lib.ptr3(uv), None, None, lib.mul3((0, 0, 0)), tc.EPS_INV,
                                                        lib.ptr(g_vd), None, lib.stream())),
        ("xeq_train_out: no channels", lambda: to._out_call(0, empty, None, a[:, :2 * F].contiguous(), None, inner, None, None, None, (F, (0, 0, 0)))),
    ]
    for message, attempt in refused:
        with pytest.raises(RuntimeError, match=message):
            attempt()
    assert lib.launch_count() == first


@pytest.mark.parametrize("prec", list(PRECISIONS))
def test_no_rows_no_launch(prec):
    """n == 0 in all four forms: outputs of the right (empty) shapes, no launch, no refusal -- the tensors of an empty batch have null
    pointers, so the entries return before they look at the cotangent and tangent pointers."""
    c, t = _small(PRECISIONS[prec], 0)
    F, mul = c.F, c.mul
    D, C = dims(mul)
    s, x, g_s, g_x, a, inner, g_os, g_ox, g_vd = (t(getattr(c, k)) for k in ("s", "x", "g_s", "g_x", "a", "inner", "g_os", "g_ox", "g_vd"))
    prm = [t(getattr(c, k)) for k in tc.PARAMS]
    uv = [s.new_zeros((0, 2 * m)) for m in mul]
    first = lib.launch_count()
    for reverse in (0, 1):
        for tan in (False, True):
            o = to._norm_call(reverse, s, s if tan else None, x, x if tan else None, *prm, g_s if reverse else None, g_x if reverse else None,
                              (F, mul, tc.EPS_LN, tc.EPS_EQ, 0))
            assert o[0].shape == (0, F) and o[1].shape == (0, D) and (o[2].shape == (0, 2 * F + C + mul[0]) if reverse else o[2] is None)
            o = to._uv_call(reverse, uv, uv if tan else None, g_vd if reverse else None, (mul, tc.EPS_INV))
            assert [v.shape for v in o] == [v.shape for v in uv] if reverse else o.shape == (0, 2 * C)
            o = to._out_call(reverse, uv, uv if tan else None, a, a if tan else None, inner, inner if tan else None, g_os if reverse else None,
                             g_ox if reverse else None, (F, mul))
            assert (o[1].shape, o[2].shape) == (a.shape, inner.shape) if reverse else (o[0].shape, o[1].shape) == ((0, F), (0, D))
    assert lib.launch_count() == first
