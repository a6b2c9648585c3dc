"""Guard bands around tensors: a net for stores outside a buffer and for reads past its end that reach a result.

The kernels work on fixed tiles and mask the ragged last one by hand; the caching allocator rounds every block up and packs small ones
into shared segments, so a store one row past the end, or a size function that is a tile short, lands in slack and no value test sees
it.  ``guarded()`` hands out a tensor that is a view into a larger backing store with a band of a known 32-bit pattern in front of it
and behind it, starting at the very first byte after the body; ``check()`` compares the bands with the pattern bit for bit.
``guard_allocations()`` puts every device allocation of a block of code (``torch.empty / zeros / full / empty_like / zeros_like``)
on such tensors and checks them all when the block ends.

Patterns (32-bit words, little endian):
  BAND_NAN     a quiet NaN read as f32 and, as either half of a pair, as f64; 2 146 966 225 read as int32, ~9.2e18 as int64
  BAND_FINITE  ~3e38 read as f32, ~5e303 as f64: a read past the end that is multiplied by zero leaves no trace with this band and a
               NaN with the other one -- run both and compare the bits (``fill="finite"`` / ``fill="nan"``)
  UNWRITTEN    the body of a tensor that stands for ``torch.empty``: a NaN with another payload ("never written")
No GPU is needed: everything here is tensor indexing, on whatever device the tensor lives."""
import contextlib
import os
import sys

import torch

BAND_BYTES = 128 * 1024        # a multiple of 512 B (the view keeps torch.empty's alignment: the kernels issue 16-byte loads) and more than
                               # one tile of the widest row any kernel stores (32 rows x 576 floats x 4 B = 72 KiB)
BAND_NAN = 0x7FF8BAD1
BAND_FINITE = 0x7F61B1E6       # 2.99999995e38 as f32
UNWRITTEN = 0x7FF8DEAD
_FILLS = {"nan": BAND_NAN, "finite": BAND_FINITE}
_HERE = os.path.abspath(__file__)

# the functions guard_allocations() replaces, as they were when this module was imported
_ORIG = {name: getattr(torch, name) for name in ("empty", "zeros", "full", "empty_like", "zeros_like")}


class GuardViolation(AssertionError):
    """A band no longer holds its pattern.  ``site``: file:line that allocated the tensor, ``side``: "front" / "back", ``offset``: first
    changed byte, counted from the start of that band (the back band starts at the first byte behind the tensor's last element)."""

    def __init__(self, site, side, offset, shape, dtype):
        self.site, self.side, self.offset = site, side, offset
        where = f"{offset} bytes behind the end" if side == "back" else f"{offset} bytes into the front band ({BAND_BYTES - offset} before the start)"
        super().__init__(f"{side} band of the {tuple(shape)} {dtype} tensor allocated at {site} was written: first changed byte {where}")


def _word(fill):
    return _FILLS[fill] if isinstance(fill, str) else int(fill) & 0xFFFFFFFF


_tiles = {}


def _tile(device, word, band):
    """band + 512 + 4 bytes of the repeated pattern on ``device`` (what a band is filled from and compared with)."""
    key = (str(device), word, band)
    if key not in _tiles:
        signed = word - (1 << 32) if word >= (1 << 31) else word
        _tiles[key] = _ORIG["full"](((band + 516) // 4,), signed, dtype=torch.int32, device=device).view(torch.uint8)
    return _tiles[key]


def _caller():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    while f is not None and f.f_code.co_filename.endswith("contextlib.py"):
        f = f.f_back
    return "?" if f is None else f"{f.f_code.co_filename}:{f.f_lineno}"


class Guard:
    """The backing store of one guarded tensor: [front band | body | back band (+ padding to 512 B)]."""

    def __init__(self, shape, dtype, device, fill, band, site):
        self.shape, self.dtype, self.site, self.band = tuple(shape), dtype, site, band
        self.word = _word(fill)
        numel = 1
        for d in self.shape:
            numel *= d
        self.nbytes = numel * _ORIG["empty"]((), dtype=dtype).element_size()
        total = band + -(-self.nbytes // 512) * 512 + band
        self.backing = _ORIG["empty"](total, dtype=torch.uint8, device=device)
        tile = _tile(self.backing.device, self.word, band)
        self.backing[:band].copy_(tile[:band])
        back = self.backing[band + self.nbytes:]
        phase = self.nbytes % 4     # the pattern is laid from the start of the backing store: the body may end inside a word
        back.copy_(tile[phase:phase + back.numel()])

    def body(self):
        return self.backing[self.band:self.band + self.nbytes]

    def view(self):
        return self.body().view(self.dtype).view(self.shape)

    def check(self):
        tile = _tile(self.backing.device, self.word, self.band)
        back = self.backing[self.band + self.nbytes:]
        phase = self.nbytes % 4
        for side, got, want in (("front", self.backing[:self.band], tile[:self.band]), ("back", back, tile[phase:phase + back.numel()])):
            if got.dtype == torch.uint8 and got.numel() % 4 == 0 and got.storage_offset() % 4 == 0 and want.storage_offset() % 4 == 0:
                if torch.equal(got.view(torch.int32), want.view(torch.int32)):     # bitwise: integer views
                    continue
            bad = torch.nonzero(got != want)
            if bad.numel():
                raise GuardViolation(self.site, side, int(bad[0, 0]), self.shape, self.dtype)


def guarded(shape, dtype=torch.float32, device="cpu", fill="nan", body="unwritten", band=BAND_BYTES):
    """A contiguous tensor of ``shape`` between two bands.  ``fill``: "nan" / "finite" (or a 32-bit word) for the bands.  ``body``:
    "unwritten" pre-fills the tensor with the never-written NaN (a stand-in for torch.empty), a number fills it with that value, None
    leaves it as the allocator gave it."""
    assert band % 512 == 0 and band > 0
    if isinstance(shape, int):
        shape = (shape,)
    g = Guard(shape, dtype, device, fill, band, _caller())
    t = g.view()
    if isinstance(body, str):
        assert body == "unwritten"
        raw = g.body()
        if g.nbytes % 4 == 0:
            raw.view(torch.int32).fill_(UNWRITTEN - (1 << 32) if UNWRITTEN >= (1 << 31) else UNWRITTEN)
        else:
            raw.fill_(0xAD)
    elif body is not None:
        t.fill_(body)
    t._guard = g
    return t


def guarded_copy(src, fill="nan", band=BAND_BYTES):
    """``src``'s values in a guarded contiguous tensor on the same device."""
    t = guarded(tuple(src.shape), src.dtype, src.device, fill=fill, body=None, band=band)
    t.copy_(src)
    return t


def guard_of(t):
    g = getattr(t, "_guard", None)
    if g is None:
        raise TypeError("not a tensor from guarded()")
    return g


def check(*tensors):
    """Both bands of every tensor against the pattern, bit for bit; raises GuardViolation (site, side, first changed byte)."""
    for t in tensors:
        guard_of(t).check()


def unwritten(t):
    """Boolean mask of the elements of a 4- or 8-byte tensor that still hold the never-written pattern."""
    size = t.element_size()
    assert size in (4, 8)
    words = t.contiguous().view(torch.int32).reshape(-1, size // 4)
    signed = UNWRITTEN - (1 << 32) if UNWRITTEN >= (1 << 31) else UNWRITTEN
    return (words == signed).all(1).reshape(t.shape)


# --------------------------------------------------------------------------------------------------------------- the interposer
def _size_of(args, kwargs):
    if "size" in kwargs:
        return tuple(kwargs.pop("size")), ()
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(int(d) for d in args[0]), ()
    if all(isinstance(a, int) or (isinstance(a, torch.Tensor) and a.dim() == 0) for a in args):
        return tuple(int(a) for a in args), ()
    return None, args


def _passes_through(device, kwargs, allowed):
    """CPU, pinned, captured and exotic allocations are not guarded."""
    if set(kwargs) - allowed:
        return True
    if kwargs.get("pin_memory") or kwargs.get("layout", torch.strided) != torch.strided:
        return True
    if kwargs.get("memory_format", torch.contiguous_format) not in (torch.contiguous_format, torch.preserve_format):
        return True
    if device.type == "cpu" or device.type == "meta":
        return True
    if device.type == "cuda" and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        return True     # a fill inside a capture would be recorded into the graph
    return False


def _default_device():
    get = getattr(torch, "get_default_device", None)
    return get() if get is not None else torch.device("cpu")


def _device(d):
    if d is None:
        return _default_device()
    d = torch.device("cuda", d) if isinstance(d, int) else torch.device(d)
    if d.type == "cuda" and d.index is None and torch.cuda.is_available():
        d = torch.device("cuda", torch.cuda.current_device())
    return d


_DTYPES = {torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64, torch.bool}
_NEW = {"dtype", "device", "requires_grad", "pin_memory", "layout", "memory_format"}


class guard_allocations(contextlib.AbstractContextManager):
    """Within the block, device allocations through torch.empty / zeros / full / empty_like / zeros_like are guarded tensors; at the end
    the device is synchronised, every band checked and the functions restored (restored also when the block raises).  ``fill`` as in
    guarded().  ``records``: the Guard of every allocation made, ``count``: how many."""

    def __init__(self, fill="nan", band=BAND_BYTES):
        self.fill, self.band = fill, band
        self.records = []
        self._saved = None

    @property
    def count(self):
        return len(self.records)

    def _make(self, shape, dtype, device, body, requires_grad):
        g = Guard(shape, dtype, device, self.fill, self.band, _caller())
        self.records.append(g)
        t = g.view()
        if body == "unwritten":
            raw = g.body()
            if g.nbytes % 4 == 0:
                raw.view(torch.int32).fill_(UNWRITTEN - (1 << 32) if UNWRITTEN >= (1 << 31) else UNWRITTEN)
            else:
                raw.fill_(0xAD)
        else:
            t.fill_(body)
        t._guard = g
        return t.requires_grad_() if requires_grad else t

    def _plain(self, name, body_of):
        orig = self._saved[name]

        def fn(*args, **kwargs):
            kw = dict(kwargs)
            shape, rest = _size_of(args, kw)
            device = _device(kw.get("device"))
            dtype = kw.get("dtype") or torch.get_default_dtype()
            if shape is None or rest or _passes_through(device, kw, _NEW) or dtype not in _DTYPES:
                return orig(*args, **kwargs)
            return self._make(shape, dtype, device, body_of, kw.get("requires_grad", False))

        fn.__name__ = name
        fn.__wrapped__ = orig
        return fn

    def _full(self):
        orig = self._saved["full"]

        def full(*args, **kwargs):
            kw = dict(kwargs)
            pos = list(args)
            if ("size" in kw) + ("fill_value" in kw) + len(pos) != 2:
                return orig(*args, **kwargs)
            shape = kw.pop("size") if "size" in kw else pos.pop(0)
            value = kw.pop("fill_value") if "fill_value" in kw else pos.pop(0)
            device = _device(kw.get("device"))
            dtype = kw.get("dtype")
            if dtype is None and not isinstance(value, torch.Tensor):
                dtype = torch.bool if isinstance(value, bool) else torch.int64 if isinstance(value, int) else torch.get_default_dtype() if isinstance(value, float) else None
            if (isinstance(value, torch.Tensor) or not isinstance(shape, (tuple, list, torch.Size)) or dtype not in _DTYPES
                    or _passes_through(device, kw, _NEW)):
                return orig(*args, **kwargs)
            return self._make(tuple(int(d) for d in shape), dtype, device, value, kw.get("requires_grad", False))

        full.__wrapped__ = orig
        return full

    def _like(self, name, body_of):
        orig = self._saved[name]

        def fn(input, **kwargs):
            if not isinstance(input, torch.Tensor) or type(input) is not torch.Tensor and not isinstance(input, torch.nn.Parameter):
                return orig(input, **kwargs)
            device = _device(kwargs.get("device", input.device))
            dense = input.layout == torch.strided and input.is_contiguous() and not input.is_quantized
            if not dense or _passes_through(device, kwargs, _NEW):
                return orig(input, **kwargs)     # a *_like of a strided input follows its strides: left to the allocator
            dtype = kwargs.get("dtype") or input.dtype
            if dtype not in _DTYPES:
                return orig(input, **kwargs)
            return self._make(tuple(input.shape), dtype, device, body_of, kwargs.get("requires_grad", False))

        fn.__name__ = name
        fn.__wrapped__ = orig
        return fn

    def __enter__(self):
        self._saved = {name: getattr(torch, name) for name in _ORIG}
        torch.empty = self._plain("empty", "unwritten")
        torch.zeros = self._plain("zeros", 0)
        torch.full = self._full()
        torch.empty_like = self._like("empty_like", "unwritten")
        torch.zeros_like = self._like("zeros_like", 0)
        return self

    def check(self):
        if any(g.backing.is_cuda for g in self.records):
            torch.cuda.synchronize()
        for g in self.records:
            g.check()

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is None:
                self.check()
        finally:
            for name, f in self._saved.items():
                setattr(torch, name, f)
        return False
