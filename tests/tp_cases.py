"""Cases, f64 / f32 references, restated host choices and restated defects for the general tensor-product kernels
(csrc/xeq_tp.hip behind xequinet_amd/tp.py::TensorProduct: k_tp_path, k_tp_fused, k_tp_tied, k_tp_wgrad).  CPU only; no test functions
here.  tests/test_gpu_tp.py runs the cases on the GPU; tests/test_tp_cases_host.py checks the reference against a direct einsum, the
properties of the case list, the restated rules against the library's query and the POWER of the bounds on the host.

A case is (irreps, instructions -- explicit or get_feasible_tp's --, weights: none / shared / one set per sample, n rows).  ``build``
draws the inputs and a cotangent G (every tensor from a stream of its own, in f64, rounded to f32 once: the f32 and the f64 run see the
same numbers), runs oracle/tp_oracle.py::tensor_product in f64 and in f32 and differentiates L = <out, G> by autograd:
``ref`` / ``ref32``: name -> tensor for out, grad_x1, grad_x2, grad_w (whichever the case has).

Bounds, per output:
  f64  1e-12 of the output's largest entry for values, 1e-11 for gradients (the figures of tests/test_tp.py);
  f32  max(4 x the f32 oracle's own error against the f64 oracle on the same inputs, 4 ulp of the output's largest entry), the rule of
       tests/test_gpu_train_edge.py.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import tp_oracle as tpo
from xequinet_amd import tp

OUTPUTS = ("out", "grad_x1", "grad_x2", "grad_w")
TIED_MODES = ("uuu", "uuw", "uvu", "uvv")
# forward mode -> (mode of the pass that writes dL/dx1, mode of the pass that writes dL/dx2): the transposed contractions
REVERSE_MODE = {"uvw": ("uvw", "uvw"), "uvu": ("uvu", "uuw"), "uvv": ("uuw", "uvv"), "uuw": ("uvv", "uvu"), "uuu": ("uuu", "uuu")}
N_WEIGHTS = {"uvw": lambda a, b, o: a * b * o, "uvu": lambda a, b, o: a * b, "uvv": lambda a, b, o: a * b, "uuw": lambda a, b, o: a * o,
             "uuu": lambda a, b, o: a, "uvuv": lambda a, b, o: a * b}
PASSES = {"fwd": "out", "dx1": "grad_x1", "dx2": "grad_x2"}


# ---------------------------------------------------------------------------------------------------- the host's choices, restated
LDS_BYTES, TILE_MAX, MIN_GROUPS, W_BLOCK, LANES, WAVES = 60000, 16, 1024, 4, 64, 4
CHUNK_ROWS, CHUNKS_MAX, GRID_Y = 64, 512, 65535
MAX_PATHS, MAX_BLOCKS = 40, 16


def tile_start(dim1, dim2, table_floats, esize):
    """Rows of x1 | x2 that fit the LDS tile behind the 3j tables, at most 16; 0: not one."""
    row, fixed = (dim1 + dim2) * esize, table_floats * esize
    return 0 if fixed + row > LDS_BYTES else min(TILE_MAX, (LDS_BYTES - fixed) // row)


def tile(n, dim1, dim2, table_floats, esize):
    """The node tile of k_tp_fused: the start, halved (rounding up) while fewer than 1024 workgroups would start."""
    tn = tile_start(dim1, dim2, table_floats, esize)
    while tn > 1 and -(-n // tn) < MIN_GROUPS:
        tn = (tn + 1) // 2
    return tn


def chunk_plan(n, shared):
    """The weight gradient's launch plan.  shared: (chunks, rows per chunk, trailing chunks without a row); per sample: the gridDim.y
    pieces [(first row, rows), ...]."""
    if shared:
        chunks = min(-(-n // CHUNK_ROWS), CHUNKS_MAX)
        rows = -(-n // chunks)
        return chunks, rows, chunks - -(-n // rows)
    return [(r, min(GRID_Y, n - r)) for r in range(0, n, GRID_Y)]


def pass_paths(c, kind):
    """The paths of a pass as the host tables them: (block the path writes, mode of the pass, mul of that block, l1, l2, l3), sorted by block
    (stable); None when the pass has no fused table ('uvuv' has no reverse)."""
    rows = []
    for k, (i1, i2, io, mode, *_) in enumerate(c.ins):
        l1, l2, l3 = c.in1[i1][1].l, c.in2[i2][1].l, c.out[io][1].l
        if kind == "fwd":
            rows.append((io, k, mode, c.out[io][0], l1, l2, l3))
        elif mode not in REVERSE_MODE:
            return None
        elif kind == "dx1":
            rows.append((i1, k, REVERSE_MODE[mode][0], c.in1[i1][0], l3, l2, l1))
        else:
            rows.append((i2, k, REVERSE_MODE[mode][1], c.in2[i2][0], l1, l3, l2))
    rows.sort(key=lambda r: (r[0], r[1]))
    return [(r[0], *r[2:]) for r in rows]


def pass_dims(c, kind):
    d1, d2, do = c.in1.dim, c.in2.dim, c.out.dim
    return {"fwd": (d1, d2), "dx1": (do, d2), "dx2": (d1, do)}[kind]


def form(c, kind, esize):
    """-> ("tied", 0) / ("tile", tile size; 0: the rows do not fit) / ("path", 0): one launch per instruction (no table: more than 40 paths
    or 16 written blocks, or a tile that does not fit)."""
    paths = pass_paths(c, kind)
    if paths is None or len(paths) > MAX_PATHS or len({p[0] for p in paths}) > MAX_BLOCKS:
        return "path", 0
    if any(len({p[1] in ("uvw", "uuw") for p in paths if p[0] == blk}) > 1 for blk in {p[0] for p in paths}):
        return "path", 0          # a block of four w and single elements cannot share an output block
    tied = all(p[1] in TIED_MODES and max(p[3:]) <= 4 for p in paths)
    for blk in {p[0] for p in paths}:
        tied = tied and len({p[1] == "uuw" for p in paths if p[0] == blk}) == 1
    if tied:
        return "tied", 0
    floats = sum((2 * p[3] + 1) * (2 * p[4] + 1) * (2 * p[5] + 1) for p in paths)
    tn = tile(c.n, *pass_dims(c, kind), floats, esize)
    return ("tile", tn) if tn else ("path", 0)


def forms(c, esize):
    return {kind: form(c, kind, esize) for kind in (PASSES if c.grads else ("fwd",))}


def pad_for_tile(in1, in2, out, ins, want, esize=8):
    """Multiplicity of a trailing 0e block of x1 that no instruction reads which makes the forward pass START at a tile of ``want``
    (0: not one row fits)."""
    probe = SimpleNamespace(in1=tp.Irreps(in1), in2=tp.Irreps(in2), out=tp.Irreps(out), ins=ins)
    floats = sum((2 * p[3] + 1) * (2 * p[4] + 1) * (2 * p[5] + 1) for p in pass_paths(probe, "fwd"))
    d1, d2 = probe.in1.dim, probe.in2.dim
    assert tile_start(d1, d2, floats, esize) > want
    pad = 1
    while tile_start(d1 + pad, d2, floats, esize) > want:
        pad += 1
    assert tile_start(d1 + pad, d2, floats, esize) == want
    return pad


# ---------------------------------------------------------------------------------------------------------------------- the cases
def _lp(irr):
    return [(m, ir.l) for m, ir in irr]


def channel_of(irr):
    """Multiplicity index u of every element of a row."""
    return torch.tensor([u for m, ir in irr for u in range(m) for _ in range(ir.dim)], dtype=torch.long)


def block_of(irr):
    """Irrep block of every element of a row."""
    return torch.tensor([b for b, (m, ir) in enumerate(irr) for _ in range(m * ir.dim)], dtype=torch.long)


def make(name, in1, in2, flt, mode, weights, n, ins=None, out=None, grads=True, dtypes=("f64", "f32"), tags=(), master=None):
    """A case.  ``flt``: get_feasible_tp's filter (then ``ins`` / ``out`` come from it) or None with explicit ``ins`` and ``out``.
    ``master``: name of a case with per-sample weights on the same product and more rows, whose first n rows this case is (with a weight
    set per row every quantity is the row's own: the slice of the master's reference is this case's reference)."""
    in1, in2 = tp.Irreps(in1), tp.Irreps(in2)
    if ins is None:
        out, ins = tp.get_feasible_tp(in1, in2, tp.Irreps(flt), mode, trainable=weights != "none")
    ins = [tuple(i) for i in ins]
    return SimpleNamespace(name=name, in1=in1, in2=in2, out=tp.Irreps(out), ins=ins, mode=mode, weights=weights, n=n,
                           grads=grads and mode != "uvuv", dtypes=tuple(dtypes), tags=tuple(tags), master=master)


def weight_layout(c):
    """[(first weight, (mul1, mul2, mul_out), mode) or None per instruction], total."""
    res, off = [], 0
    for i1, i2, io, mode, has_w, *_ in c.ins:
        if not has_w:
            res.append(None)
            continue
        m = (c.in1[i1][0], c.in2[i2][0], c.out[io][0])
        res.append((off, m, mode))
        off += N_WEIGHTS[mode](*m)
    return res, off


def outputs(c):
    if not c.grads:
        return ("out",)
    return OUTPUTS if c.weights != "none" else OUTPUTS[:3]


def _draw(c, k, *shape):
    seed = [2031, k, *[ord(ch) for ch in c.name]]
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape)).float().double()


def inputs(c):
    """x1, x2, w (None / [W] / [n, W]) and the cotangent G, f64 holding f32-representable numbers."""
    W = weight_layout(c)[1]
    w = None if c.weights == "none" else _draw(c, 2, W) if c.weights == "shared" else _draw(c, 2, c.n, W)
    return _draw(c, 0, c.n, c.in1.dim), _draw(c, 1, c.n, c.in2.dim), w, _draw(c, 3, c.n, c.out.dim)


def oracle(c, x, y, w, G, dtype, ins=None, w3j=tp.wigner_3j):
    """oracle/tp_oracle.py on the case in ``dtype`` -> name -> tensor (f64 on return), gradients by autograd of <out, G>."""
    t = lambda v: None if v is None else v.to(dtype).clone().requires_grad_(c.grads)
    x, y, w, G = t(x), t(y), t(w), G.to(dtype)
    res = tpo.tensor_product(_lp(c.in1), _lp(c.in2), _lp(c.out), c.ins if ins is None else ins, w3j, x, y, w, shared_weights=c.weights != "sample")
    got = {"out": res.detach().double()}
    if c.grads:
        leaves = [v for v in (x, y, w) if v is not None]
        for name, g in zip(outputs(c)[1:], torch.autograd.grad((res * G).sum(), leaves, allow_unused=True)):
            got[name] = (torch.zeros_like(leaves[outputs(c)[1:].index(name)]) if g is None else g).double()
    return got


_BUILT = {}


def build(c):
    """The case with inputs (x, y, w, G) and ref / ref32; kept by name, computed once, never modified."""
    if c.master is not None:
        m = build(by_name(c.master))
        assert c.weights == m.weights == "sample" and c.n <= m.n and c.ins == m.ins and (c.in1, c.in2, c.out) == (m.in1, m.in2, m.out)
        b = SimpleNamespace(**vars(c))
        b.x, b.y, b.w, b.G = (v[:c.n] for v in (m.x, m.y, m.w, m.G))
        b.ref, b.ref32 = ({k: v[:c.n] for k, v in r.items()} for r in (m.ref, m.ref32))
        return b
    if c.name not in _BUILT:
        b = SimpleNamespace(**vars(c))
        b.x, b.y, b.w, b.G = inputs(c)
        b.ref = oracle(c, b.x, b.y, b.w, b.G, torch.float64)
        b.ref32 = oracle(c, b.x, b.y, b.w, b.G, torch.float32)
        _BUILT[c.name] = b
    return _BUILT[c.name]


def forget(c):
    """Drop a built case (the long ones hold hundreds of megabytes)."""
    _BUILT.pop(c.name, None)


def module(c):
    """The TensorProduct of the case; weights are always passed in."""
    return tp.TensorProduct(c.in1, c.in2, c.out, c.ins, internal_weights=False, shared_weights=c.weights != "sample")


IN_A, IN_B = "6x0e+6x1o+6x2e", "3x0e+5x1o+2x2e"                    # tests/test_tp.py::_case
IN_SA, IN_SB = "3x0e+3x1o+3x2e", "1x0e+2x1o+1x2e"                   # the same kinds of paths on fewer channels
FLT_6 = "6x0e+6x1o+6x1e+6x2e+6x3o"                                  # 1 836 weights in 'uvw'
FLT_145 = "1x0e+4x1o+5x1e+1x2e+5x3o"                                # output multiplicities at the edges of the blocks of four w
FLT_ANY = "1x0e+1x1o+1x1e+1x2e+1x2o+1x3o+1x4e"
TILE_ROWS = (1, 2046, 2047, 4094, 8186, 16370)                      # tiles 1, 1, 2, 4, 8, 16; the last four end in a partial tile
ODD_ROWS = ((5118, 5, 3), (3071, 3, 2))                             # (n, tile, rows of the last tile) from an LDS-limited start of 5
TIED_MULS = (1, 63, 64, 65, 129)
TIED_ROWS = (1, 3, 4, 5, 9)                                         # four waves per workgroup, a wave per node
WGRAD_ROWS = (1, 64, 65, 129, 32768, 32769)
SAMPLE_ROWS = 65537


def _hidden(m):
    return f"{m}x0e+{m}x1o+{m}x2e"


def reference_products(ch):
    """The two general products the reference builds: SelfMixTP's 'uuu' (l up to 4) and the Cartesian-tensor head's 'uuw' ch -> 1."""
    hid = tp.Irreps([(ch, (l, (-1) ** l)) for l in range(3)])
    mix = [(ch, (0, 1))] + [(ch, (l, s)) for l in range(2, 4) for s in (-1, 1)] + [(ch, (4, 1))]
    out, ins = tp.get_feasible_tp(hid, hid, tp.Irreps(mix), "uuu")
    out2, ins2 = tp.get_feasible_tp(out, out, tp.Irreps("1x0e+1x2e"), "uuw")
    return (hid, hid, out, ins), (out, out, out2, ins2)


@functools.lru_cache(maxsize=None)
def cases():
    cs = []
    # ---- tile form, 'uvw': every tile size from the default start, both weight kinds, both sets of output multiplicities.  With a weight
    # set per row the oracle's einsum takes 13 s for 16 370 rows of 1 836 weights (7 s for 912): those products run at the rows of tiles
    # 1, 1, 2, and the rows of tiles 4, 8, 16 run a product of the same kind with 3 | 1, 2, 1 input channels (228 weights per row),
    # all three row counts as slices of one 16 370-row reference.
    for tag, flt in (("m6", FLT_6), ("m145", FLT_145)):
        for n in TILE_ROWS:
            cs.append(make(f"uvw-{tag}-shared-n{n}", IN_A, IN_B, flt, "uvw", "shared", n, tags=("tile",)))
        for n in TILE_ROWS[:3]:
            cs.append(make(f"uvw-{tag}-sample-n{n}", IN_A, IN_B, flt, "uvw", "sample", n, tags=("tile",)))
    for n in TILE_ROWS[:2:-1]:
        cs.append(make(f"uvw-s145-sample-n{n}", IN_SA, IN_SB, FLT_145, "uvw", "sample", n, tags=("tile",),
                       master=None if n == TILE_ROWS[-1] else f"uvw-s145-sample-n{TILE_ROWS[-1]}"))
    # ---- odd tiles, f64: rows of x1 padded by a block no instruction reads until the LDS limit starts the forward pass at 5
    out, ins = tp.get_feasible_tp(IN_A, IN_B, tp.Irreps(FLT_145), "uvw")
    pad = pad_for_tile(IN_A, IN_B, out, ins, 5)
    for n, tn, last in ODD_ROWS:
        cs.append(make(f"uvw-m145-pad-n{n}", f"{IN_A}+{pad}x0e", IN_B, None, "uvw", "shared", n, ins=ins, out=out, dtypes=("f64",), tags=("tile", "odd")))
    # ---- tile form, 'uvuv': exactly 16 written blocks, forward only
    cs.append(make("uvuv-n16370", IN_A, IN_B, FLT_ANY, "uvuv", "none", 16370, tags=("tile",)))
    # ---- tied form
    tied = [("uuu-shared", "uuu", "shared", None, FLT_ANY), ("uuu-none", "uuu", "none", None, FLT_ANY)]
    tied += [(f"uuw-{w}-o{mo}", "uuw", w, None, "+".join(f"{mo}x{ir}" for ir in ("0e", "1o", "1e", "2e", "3o"))) for w in ("shared", "sample") for mo in (1, 3)]
    tied += [("uvu-shared", "uvu", "shared", IN_B, FLT_ANY), ("uvv-sample", "uvv", "sample", IN_B, FLT_ANY)]
    for tag, mode, weights, other, flt in tied:
        for m in TIED_MULS:
            for n in TIED_ROWS:
                in1, in2 = (_hidden(m), _hidden(m)) if other is None else (_hidden(m), other) if mode == "uvu" else (other, _hidden(m))
                cs.append(make(f"{tag}-m{m}-n{n}", in1, in2, flt, mode, weights, n, tags=("tied",)))
    (h1, h2, ho, hi), (o1, o2, oo, oi) = reference_products(65)
    cs.append(make("selfmix-m65-n5", h1, h2, None, "uuu", "shared", 5, ins=hi, out=ho, tags=("tied", "l4")))
    cs.append(make("head-m65-n5", o1, o2, None, "uuw", "sample", 5, ins=oi, out=oo, tags=("tied", "l4")))
    # ---- weight-gradient chunking
    for n in WGRAD_ROWS:
        cs.append(make(f"wgrad-uuu-m2-shared-n{n}", _hidden(2), _hidden(2), FLT_ANY, "uuu", "shared", n, tags=("wgrad",)))
    cs.append(make("wgrad-uvw-m6-shared-n129", IN_A, IN_B, FLT_6, "uvw", "shared", 129, tags=("wgrad",)))
    cs.append(make(f"wgrad-uuu-m2-sample-n{SAMPLE_ROWS}", _hidden(2), _hidden(2), FLT_ANY, "uuu", "sample", SAMPLE_ROWS, tags=("wgrad",)))
    # ---- paths into one block with DIFFERENT coefficients, one case per form
    three = [(0, 0, 0, "uuu", True, 1.0), (1, 1, 0, "uuu", True, 4.0), (2, 2, 0, "uuu", True, 0.25), (1, 1, 1, "uuu", True, 1.0)]
    cs.append(make("coeff-uuu-n5", _hidden(3), _hidden(3), None, "uuu", "shared", 5, ins=three, out="3x0e+3x2e", tags=("tied", "coeff")))
    three = [(0, 0, 0, "uvw", True, 1.0), (1, 1, 0, "uvw", True, 4.0), (2, 2, 0, "uvw", True, 0.25), (1, 1, 1, "uvw", True, 1.0)]
    cs.append(make("coeff-uvw-n5", IN_A, IN_B, None, "uvw", "shared", 5, ins=three, out="5x0e+3x2e", tags=("tile", "coeff")))
    # ---- limits: 17 written blocks and 41 paths run one launch per instruction; rows too long for the LDS tile do as well
    cs.append(make("limit-17-blocks-n5", "2x0e+2x1o", "2x0e+2x1o", None, "uuu", "shared", 5, out="+".join(["2x0e", "2x1o"] * 8 + ["2x0e"]),
                   ins=[(k % 2, 0, k, "uuu", True, 1.0) for k in range(17)], tags=("limit",)))
    cs.append(make("limit-41-paths-n5", "2x0e+2x1o", "2x0e+2x1o", None, "uuu", "shared", 5, out="2x0e+2x1o",
                   ins=[(k % 2, 0, k % 2, "uuu", True, 1.0 + k) for k in range(41)], tags=("limit",)))
    out, ins = tp.get_feasible_tp(IN_A, IN_B, tp.Irreps(FLT_145), "uvw")
    over = pad_for_tile(IN_A, IN_B, out, ins, 0)
    cs.append(make("limit-lds-n3", f"{IN_A}+{over}x0e", IN_B, None, "uvw", "shared", 3, ins=ins, out=out, dtypes=("f64",), tags=("limit",)))
    return tuple(cs)


def by_name(name):
    return next(c for c in cases() if c.name == name)


def tagged(tag):
    return [c for c in cases() if tag in c.tags]


# -------------------------------------------------------------------------------------------------------------------------- bounds
EPS32 = float(torch.finfo(torch.float32).eps)
F32_FACTOR = 4.0


def f64_tolerance(name):
    return 1e-12 if name == "out" else 1e-11


def judge(ref, ref32, got, names, f64):
    """Per output: (name, kernel error, the f32 oracle's own error, bound, largest entry).  An output that is not finite has an
    infinite error."""
    res = []
    for k in names:
        r, g = ref[k], got[k].double()
        top = float(r.abs().max()) if r.numel() else 0.0
        err = (float((g - r).abs().max()) if bool(torch.isfinite(g).all()) else float("inf")) if r.numel() else 0.0
        e32 = float((ref32[k] - r).abs().max()) if r.numel() else 0.0
        res.append((k, err, e32, f64_tolerance(k) * top if f64 else max(F32_FACTOR * e32, F32_FACTOR * EPS32 * top), top))
    return res


def broken(res):
    """Names of the outputs of ``judge`` that leave their bound."""
    return tuple(k for k, err, _, bound, _ in res if not err <= bound)


# ------------------------------------------------------------------------------------------------------------------------- defects
HOLE = float("nan")


def _elements(irr, blk, lo_mul):
    """Mask of the elements of block ``blk`` with multiplicity index >= lo_mul."""
    return (block_of(irr) == blk) & (channel_of(irr) >= lo_mul)


def _pass_target(c, kind):
    return {"fwd": c.out, "dx1": c.in1, "dx2": c.in2}[kind]


def d_last_wblock(b):
    """k_tp_fused: the last, partial block of four w of a blocked slot ('uvw' / 'uuw' passes) is not stored: it stays as the zero fill."""
    res = {k: v.clone() for k, v in b.ref.items()}
    for kind, name in PASSES.items():
        if name not in res:
            continue
        for blk, mode, mulo, *_ in pass_paths(b, kind):
            if mode in ("uvw", "uuw") and mulo % W_BLOCK:
                res[name][:, _elements(_pass_target(b, kind), blk, mulo // W_BLOCK * W_BLOCK)] = 0
    return res


def d_wblock_overrun(b):
    """k_tp_fused: the last block of four w of a blocked slot is stored whole, past mul_out: its sums for w >= mul_out are zeros, and
    behind the last block of a row they land on the first elements of the next row (behind the last row: in the guard band)."""
    res = {k: v.clone() for k, v in b.ref.items()}
    for kind, name in PASSES.items():
        if name not in res:
            continue
        target = _pass_target(b, kind)
        for blk, mode, mulo, *_ in pass_paths(b, kind):
            if mode in ("uvw", "uuw") and mulo % W_BLOCK and blk == len(target) - 1:
                res[name][1:, :(-mulo % W_BLOCK) * target[blk][1].dim] = 0
    return res


def d_last_tile(b, esize=8):
    """k_tp_fused: the partial last tile of a pass is not run: its rows stay as the zero fill."""
    res = {k: v.clone() for k, v in b.ref.items()}
    for kind, name in PASSES.items():
        f, tn = form(b, kind, esize) if name in res else ("", 0)
        if f == "tile" and b.n % tn:
            res[name][b.n // tn * tn:] = 0
    return res


def d_lanes_64(b):
    """k_tp_tied: the lanes make one round: channels >= 64 are not visited.  Output channels tied to the lane stay zero; the sum over u
    of an 'uuw' pass loses its terms u >= 64."""
    res = {k: v.clone() for k, v in b.ref.items()}
    for kind, name in PASSES.items():
        if name not in res:
            continue
        target = _pass_target(b, kind)
        for blk, mode, mulo, *_ in pass_paths(b, kind):
            if mode != "uuw":
                res[name][:, _elements(target, blk, LANES)] = 0
    if b.mode == "uuw":      # forward: the summed index is x1's channel
        x = b.x.clone()
        x[:, channel_of(b.in1) >= LANES] = 0
        res["out"] = oracle(SimpleNamespace(**{**vars(b), "grads": False}), x, b.y, b.w, b.G, torch.float64)["out"]
    return res


def _restride(flat, off, shape, other):
    """The block [rows, cols] at ``off`` of ``flat`` [..., W] read with the row stride ``other`` instead of cols; reads past the end of
    the weight vector are holes."""
    rows, cols = shape
    idx = off + torch.arange(rows)[:, None] * other + torch.arange(cols)[None, :]
    padded = torch.cat([flat, flat.new_full((*flat.shape[:-1], int(idx.max()) + 1), HOLE)], -1)
    return padded[..., idx.reshape(-1)]


def d_weight_stride(b):
    """'uuw': W[u * mul_out + w] read (and its gradient written) as W[u * mul1 + w]; 'uvu' / 'uvv': W[u * mul2 + v] as W[u * mul1 + v] --
    the stride taken from the other multiplicity, in the forward pass and in k_tp_wgrad's decoding of the weight index."""
    assert b.mode in ("uuw", "uvu", "uvv")
    w, gw = b.w.clone(), b.ref["grad_w"].clone()
    for lay in weight_layout(b)[0]:
        if lay is None:
            continue
        off, (m1, m2, mo), mode = lay
        shape = (m1, mo) if mode == "uuw" else (m1, m2)
        numel = shape[0] * shape[1]
        w[..., off:off + numel] = _restride(b.w, off, shape, m1)
        gw[..., off:off + numel] = _restride(b.ref["grad_w"], off, shape, m1)
    res = {k: v.clone() for k, v in b.ref.items()}
    res["out"] = oracle(SimpleNamespace(**{**vars(b), "grads": False}), b.x, b.y, w, b.G, torch.float64)["out"]
    res["grad_w"] = gw
    return res


def d_coeff_per_block(b):
    """The coefficient of the FIRST path of an output block is applied to the block's sum, not each path's own to its term."""
    first = {}
    for ins in b.ins:
        first.setdefault(ins[2], ins[5])
    ins = [(*i[:5], first[i[2]]) for i in b.ins]
    res = {k: v.clone() for k, v in b.ref.items()}
    res["out"] = oracle(SimpleNamespace(**{**vars(b), "grads": False}), b.x, b.y, b.w, b.G, torch.float64, ins=ins)["out"]
    return res


def d_first_table(b):
    """Every path reads the 3j tables from the first float of the staged buffer (its own offset dropped): a later path sees the first
    path's numbers in its own shape."""
    order = sorted(range(len(b.ins)), key=lambda k: (b.ins[k][2], k))
    flat = torch.cat([tp.wigner_3j(b.in1[b.ins[k][0]][1].l, b.in2[b.ins[k][1]][1].l, b.out[b.ins[k][2]][1].l).reshape(-1) for k in order])

    def w3j(l1, l2, l3):
        shape = (2 * l1 + 1, 2 * l2 + 1, 2 * l3 + 1)
        return flat[:math.prod(shape)].reshape(shape).clone()

    res = {k: v.clone() for k, v in b.ref.items()}
    res["out"] = oracle(SimpleNamespace(**{**vars(b), "grads": False}), b.x, b.y, b.w, b.G, torch.float64, w3j=w3j)["out"]
    return res


def d_empty_chunks(b):
    """k_tp_wgrad, shared weights: the threads of a chunk without rows return before their store: the caller's sum takes in whatever the
    parts buffer held."""
    res = {k: v.clone() for k, v in b.ref.items()}
    if chunk_plan(b.n, True)[2]:
        res["grad_w"] += HOLE
    return res


def d_second_piece(b):
    """k_tp_wgrad, per-sample weights: the second gridDim.y piece reads its rows one row late."""
    res = {k: v.clone() for k, v in b.ref.items()}
    for first, rows in chunk_plan(b.n, False)[1:]:
        res["grad_w"][first:first + rows - 1] = b.ref["grad_w"][first + 1:first + rows]
        res["grad_w"][first + rows - 1] = HOLE
    return res


# defect -> (the wrong function, the outputs it must move, the case meant to catch it)
DEFECTS = {
    "last_wblock": (d_last_wblock, ("out", "grad_x1", "grad_x2"), "uvw-m145-shared-n1"),
    "wblock_overrun": (d_wblock_overrun, ("out", "grad_x1", "grad_x2"), "uvw-m145-shared-n2046"),
    "last_tile": (d_last_tile, ("out", "grad_x1", "grad_x2"), "uvw-m145-shared-n2047"),
    "lanes_64_uuu": (d_lanes_64, ("out", "grad_x1", "grad_x2"), "uuu-shared-m65-n1"),
    "lanes_64_uuw": (d_lanes_64, ("out", "grad_x1", "grad_x2"), "uuw-sample-o3-m65-n1"),
    "weight_stride_uuw": (d_weight_stride, ("out", "grad_w"), "uuw-shared-o3-m63-n3"),
    "weight_stride_uvu": (d_weight_stride, ("out", "grad_w"), "uvu-shared-m63-n3"),
    "weight_stride_uvv": (d_weight_stride, ("out", "grad_w"), "uvv-sample-m63-n3"),
    "coeff_per_block_tied": (d_coeff_per_block, ("out",), "coeff-uuu-n5"),
    "coeff_per_block_tile": (d_coeff_per_block, ("out",), "coeff-uvw-n5"),
    "first_table": (d_first_table, ("out",), "uvw-m145-shared-n1"),
    "empty_chunks": (d_empty_chunks, ("grad_w",), "wgrad-uuu-m2-shared-n32769"),
    "second_piece": (d_second_piece, ("grad_w",), f"wgrad-uuu-m2-sample-n{SAMPLE_ROWS}"),
}
