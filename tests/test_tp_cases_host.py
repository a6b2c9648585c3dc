"""tests/tp_cases.py on the host: the reference against direct einsums, the properties the case list is there for, the restated host rules
(form, tile, chunks) against the library's own queries for every case, and the power of the bounds: every restated defect leaves them in
exactly the outputs it names, on the case meant to catch it, in both precisions."""
import math

import pytest
import torch

from tests import tp_cases as tc
from xequinet_amd import lib, tp

ESIZE = {"f64": 8, "f32": 4}
DTYPE = {"f64": torch.float64, "f32": torch.float32}


def _direct(b):
    """out of the case by one einsum per instruction written here, coefficients from e3nn's formula; gradients by autograd."""
    n_el = {"uvw": lambda a, c: a * c, "uuu": lambda a, c: 1}
    x, y, w = (v.clone().requires_grad_() for v in (b.x, b.y, b.w))
    o1, o2, oo = b.in1.offsets(), b.in2.offsets(), b.out.offsets()
    out, off = torch.zeros(b.n, b.out.dim, dtype=torch.float64), 0
    for i1, i2, io, mode, has_w, pw in b.ins:
        (m1, r1), (m2, r2), (mo, ro) = b.in1[i1], b.in2[i2], b.out[io]
        total = sum(n_el[k[3]](b.in1[k[0]][0], b.in2[k[1]][0]) for k in b.ins if k[2] == io)
        coeff = math.sqrt(ro.dim * pw / total)
        C = tp.wigner_3j(r1.l, r2.l, ro.l)
        xb = x[:, o1[i1]:o1[i1] + m1 * r1.dim].reshape(b.n, m1, r1.dim)
        yb = y[:, o2[i2]:o2[i2] + m2 * r2.dim].reshape(b.n, m2, r2.dim)
        if mode == "uuu":       # shared weights
            r = torch.einsum("u,ijk,nui,nuj->nuk", w[off:off + m1], C, xb, yb)
            off += m1
        else:                   # 'uvw', a weight set per row
            r = torch.einsum("nuvw,ijk,nui,nvj->nwk", w[:, off:off + m1 * m2 * mo].reshape(b.n, m1, m2, mo), C, xb, yb)
            off += m1 * m2 * mo
        out = out + torch.nn.functional.pad(coeff * r.reshape(b.n, -1), (oo[io], b.out.dim - oo[io] - mo * ro.dim))
    grads = torch.autograd.grad((out * b.G).sum(), [x, y, w])
    return dict(zip(tc.OUTPUTS, (out.detach(), *grads)))


@pytest.mark.parametrize("name", ["coeff-uuu-n5", "uvw-m145-sample-n1"])
def test_reference_is_the_direct_einsum(name):
    b = tc.build(tc.by_name(name))
    want = _direct(b)
    for k in tc.OUTPUTS:
        assert b.ref[k].shape == want[k].shape and float((b.ref[k] - want[k]).abs().max()) <= 1e-13 * float(want[k].abs().max()), k
        assert 0 < float((b.ref32[k] - want[k]).abs().max()) <= 1e-5 * float(want[k].abs().max()), k      # f32 is f32, and no worse


def test_inputs_are_f32_numbers_and_slices_of_a_master_are_the_masters_rows():
    c = tc.by_name("uvw-s145-sample-n4094")
    b, m = tc.build(c), tc.build(tc.by_name(c.master))
    for v in (b.x, b.y, b.w, b.G):
        assert v.dtype == torch.float64 and torch.equal(v, v.float().double())
    direct = tc.oracle(c, b.x[:7], b.y[:7], b.w[:7], b.G[:7], torch.float64)
    for k in tc.OUTPUTS:
        assert torch.equal(b.ref[k], m.ref[k][:c.n]) and float((direct[k] - b.ref[k][:7]).abs().max()) <= 1e-13 * float(b.ref[k].abs().max())


def test_case_list_reaches_every_edge_it_is_there_for():
    cs = tc.cases()
    assert len({c.name for c in cs}) == len(cs)
    tiles, partial, kinds = set(), set(), set()
    for c in cs:
        for prec in c.dtypes:
            for kind, (f, tn) in tc.forms(c, ESIZE[prec]).items():
                kinds.add(f)
                if f == "tile":
                    tiles.add(tn)
                    if c.n % tn:
                        partial.add(tn)
    assert tiles == {1, 2, 3, 4, 5, 8, 16} and partial == tiles - {1} and kinds == {"tied", "tile", "path"}
    for n, tn, last in tc.ODD_ROWS:      # the odd tiles come from the forward pass of the padded case, with the partial tiles announced
        c = tc.by_name(f"uvw-m145-pad-n{n}")
        assert tc.form(c, "fwd", 8) == ("tile", tn) and n % tn == last and c.in1[-1][0] > 1000
        assert not any(i[0] == len(c.in1) - 1 for i in c.ins)
    assert [tc.form(tc.by_name(f"uvw-m6-shared-n{n}"), "fwd", 4)[1] for n in tc.TILE_ROWS] == [1, 1, 2, 4, 8, 16]
    assert len({i[2] for i in tc.by_name("uvuv-n16370").ins}) == 16
    # every mode with unequal multiplicities (for the tied pairs u = v: input against output)
    unequal = set()
    for c in cs:
        for i1, i2, io, mode, *_ in c.ins:
            m1, m2, mo = c.in1[i1][0], c.in2[i2][0], c.out[io][0]
            if {"uvw": len({m1, m2, mo}) == 3, "uuw": mo != m1, "uuu": False}.get(mode, m1 != m2):
                unequal.add(mode)
    assert unequal == {"uvw", "uvu", "uvv", "uuw", "uvuv"} and any(c.mode == "uuu" for c in cs)
    for tag in ("uuu-shared", "uuu-none", "uuw-shared-o1", "uuw-shared-o3", "uuw-sample-o1", "uuw-sample-o3", "uvu-shared", "uvv-sample"):
        for m in tc.TIED_MULS:
            for n in tc.TIED_ROWS:
                c = tc.by_name(f"{tag}-m{m}-n{n}")
                assert set(tc.forms(c, 4).values()) == {("tied", 0)} and m in {mul for mul, _ in (*c.in1, *c.in2)}
    assert max(ir.l for _, ir in tc.by_name("selfmix-m65-n5").out) == 4
    # the weight gradient's plans
    assert [tc.chunk_plan(n, True) for n in tc.WGRAD_ROWS] == [(1, 1, 0), (1, 64, 0), (2, 33, 0), (3, 43, 0), (512, 64, 0), (512, 65, 7)]
    assert tc.chunk_plan(tc.SAMPLE_ROWS, False) == [(0, 65535), (65535, 2)]
    assert {c.n for c in tc.tagged("wgrad") if c.weights == "shared" and c.mode == "uuu"} == set(tc.WGRAD_ROWS)
    assert tc.by_name(f"wgrad-uuu-m2-sample-n{tc.SAMPLE_ROWS}").weights == "sample" and tc.weight_layout(tc.by_name("wgrad-uvw-m6-shared-n129"))[1] == 1836
    # the limits
    assert tc.form(tc.by_name("limit-17-blocks-n5"), "fwd", 8) == ("path", 0) and len({i[2] for i in tc.by_name("limit-17-blocks-n5").ins}) == 17
    assert set(tc.forms(tc.by_name("limit-41-paths-n5"), 8).values()) == {("path", 0)} and len(tc.by_name("limit-41-paths-n5").ins) == 41
    assert tc.forms(tc.by_name("limit-lds-n3"), 8) == {"fwd": ("path", 0), "dx1": ("tile", 1), "dx2": ("path", 0)}


def test_restated_form_tile_and_chunk_rules_are_the_librarys():
    """xeq_tensor_product_form (the function the launch itself calls) and xeq_tensor_product_wgrad_chunks for every case, pass and
    precision; 'path' is the host's: no table, or a table whose form is 0."""
    L = lib.load()
    mods = {}
    for c in tc.cases():
        key = (repr(c.in1), repr(c.in2), repr(c.out), tuple(c.ins), c.weights)
        mod = mods.setdefault(key, tc.module(c))
        dims = {"fwd": (c.in1.dim, c.in2.dim), "dx1": (c.out.dim, c.in2.dim), "dx2": (c.in1.dim, c.out.dim)}
        for prec in ("f64", "f32"):
            like = torch.empty(0, dtype=DTYPE[prec])
            for kind in ("fwd", "dx1", "dx2"):
                want = tc.form(c, kind, ESIZE[prec])
                t = mod._fused_table(kind, like)
                if t is None:
                    got = ("path", 0)
                else:
                    a, b = (torch.empty((c.n, d), dtype=DTYPE[prec], device="meta") for d in dims[kind])
                    f = mod.pass_form(t, a, b)
                    got = ("tied", 0) if f == -1 else ("tile", f) if f > 0 else ("path", 0)
                    assert (mod._pass_table(kind, a, b) is None) == (f == 0)
                assert got == want, (c.name, prec, kind, got, want)
        assert L.xeq_tensor_product_wgrad_chunks(c.n) == tc.chunk_plan(c.n, True)[0]
    # the tile rule away from the cases: every start, row counts around every halving
    mod = tc.module(tc.by_name("uvw-m145-shared-n1"))
    t = mod._fused_table("fwd", torch.empty(0, dtype=torch.float64))
    for dim1 in (54, 400, 700, 1110, 1500, 2400, 3700, 7000, 7500):
        for n in (1, 1023, 1024, 1025, 2047, 2048, 3070, 3071, 3072, 4093, 5115, 5116, 8185, 16368, 16369, 100000):
            for dtype, esize in ((torch.float64, 8), (torch.float32, 4)):
                got = L.xeq_tensor_product_form(lib.dtype_code(torch.empty(0, dtype=dtype)), n, dim1, 28, t["n_paths"], t["paths"], t["cg_floats"])
                assert got == tc.tile(n, dim1, 28, t["cg_floats"], esize), (dim1, n, esize)
    assert L.xeq_tensor_product_form(lib.XEQ_F64, 5, 54, 28, 0, t["paths"], t["cg_floats"]) == 0 and b"xeq_tensor_product_form" in L.xeq_last_error()


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("defect", list(tc.DEFECTS))
def test_every_defect_leaves_the_bounds_in_exactly_the_outputs_it_names(defect, prec):
    fn, names, case = tc.DEFECTS[defect]
    b = tc.build(tc.by_name(case))
    assert prec in b.dtypes
    got = fn(b)
    assert tc.broken(tc.judge(b.ref, b.ref32, got, tc.outputs(b), prec == "f64")) == names
    for k in tc.outputs(b):
        if k not in names:
            assert torch.equal(got[k], b.ref[k])
    # the oracle's own f32 run is inside the f32 bounds, and the exact result inside both
    assert tc.broken(tc.judge(b.ref, b.ref32, b.ref32, tc.outputs(b), False)) == ()
    assert tc.broken(tc.judge(b.ref, b.ref32, b.ref, tc.outputs(b), prec == "f64")) == ()


def test_a_square_product_cannot_see_the_weight_stride():
    """Why the 6 -> 6 'uuw' product of tests/test_tp.py is not enough: with mul_out == mul1 the wrong stride is the right one."""
    sq = tc.make("square-uuw", tc.IN_A, tc.IN_A, tc.FLT_6, "uuw", "shared", 3)
    b = tc.SimpleNamespace(**vars(sq))
    b.x, b.y, b.w, b.G = tc.inputs(sq)
    b.ref = tc.oracle(sq, b.x, b.y, b.w, b.G, torch.float64)
    got = tc.d_weight_stride(b)
    assert all(torch.equal(got[k], b.ref[k]) for k in tc.OUTPUTS)
