"""The guard-band helper (tests/guard_bands.py) on CPU tensors: layout of the view, the checker's report for a one-byte change at
either end, and what guard_allocations() replaces, passes through and restores.  Violations are planted with ordinary tensor indexing
on the backing store."""
import os

import pytest
import torch

from tests import guard_bands as gb

NAMES = ("empty", "zeros", "full", "empty_like", "zeros_like")


@pytest.mark.parametrize("shape,dtype", [((33, 576), torch.float32), ((7,), torch.float64), ((5, 3), torch.int64), ((13,), torch.int32),
                                         ((3, 7), torch.uint8), ((0, 128), torch.float32), ((), torch.float32)])
def test_view_is_contiguous_aligned_and_sits_between_the_bands(shape, dtype):
    t = gb.guarded(shape, dtype, "cpu")
    g = gb.guard_of(t)
    assert t.shape == torch.Size(shape) and t.dtype == dtype and t.is_contiguous()
    assert gb.BAND_BYTES % 512 == 0 and gb.BAND_BYTES >= 32 * 576 * 4
    assert t.storage_offset() * t.element_size() == gb.BAND_BYTES        # a multiple of 512 B behind the allocator's own alignment
    if t.numel():
        assert t.data_ptr() - g.backing.data_ptr() == gb.BAND_BYTES and t.data_ptr() % 16 == 0
    assert g.backing.numel() >= 2 * gb.BAND_BYTES + t.numel() * t.element_size()
    assert (g.backing.numel() - gb.BAND_BYTES - g.nbytes) >= gb.BAND_BYTES
    gb.check(t)


def test_patterns_read_as_nan_and_as_absurd_indices():
    t = gb.guarded((4,), torch.float32, "cpu", fill="nan")
    g = gb.guard_of(t)
    front = g.backing[:gb.BAND_BYTES]
    assert torch.isnan(front.view(torch.float32)).all() and torch.isnan(front.view(torch.float64)).all()
    assert int(front.view(torch.int32)[0]) == gb.BAND_NAN > 2 ** 30 and int(front.view(torch.int64)[0]) > 2 ** 60
    assert torch.isnan(t).all() and gb.unwritten(t).all()                 # the body of a torch.empty stand-in: the other NaN
    assert int(t.view(torch.int32)[0]) == gb.UNWRITTEN != gb.BAND_NAN
    d = gb.guarded((4,), torch.float64, "cpu")
    assert torch.isnan(d).all() and gb.unwritten(d).all()
    f = gb.guarded((4,), torch.float32, "cpu", fill="finite", body=0.0)
    band = gb.guard_of(f).backing[-gb.BAND_BYTES:]
    assert torch.isfinite(band.view(torch.float32)).all() and float(band.view(torch.float32)[0]) > 1e38
    assert torch.isfinite(band.view(torch.float64)).all() and float(band.view(torch.float64)[0]) > 1e300
    assert (f == 0).all() and not gb.unwritten(f).any()


def test_writing_the_whole_body_leaves_the_bands_intact():
    for dtype in (torch.float32, torch.uint8, torch.int64):
        t = gb.guarded((17, 3), dtype, "cpu")
        t.fill_(1)
        gb.check(t)
        assert not gb.unwritten(t).any() if dtype != torch.uint8 else True


@pytest.mark.parametrize("side,where", [("front", 0), ("front", gb.BAND_BYTES - 1), ("back", 0), ("back", 5), ("back", "last")])
@pytest.mark.parametrize("shape,dtype", [((33, 5), torch.float32), ((3, 7), torch.uint8)])
def test_one_changed_byte_is_reported_with_side_and_offset(side, where, shape, dtype):
    t = gb.guarded(shape, dtype, "cpu")
    g = gb.guard_of(t)
    start = 0 if side == "front" else gb.BAND_BYTES + g.nbytes
    length = gb.BAND_BYTES if side == "front" else g.backing.numel() - start
    off = length - 1 if where == "last" else where
    g.backing[start + off] ^= 0x01                                           # one bit of one byte
    with pytest.raises(gb.GuardViolation) as e:
        gb.check(t)
    assert e.value.side == side and e.value.offset == off
    site_file, site_line = e.value.site.rsplit(":", 1)
    assert os.path.samefile(site_file, __file__) and int(site_line) > 0 and side in str(e.value) and e.value.site in str(e.value)
    g.backing[start + off] ^= 0x01
    gb.check(t)


def test_a_store_one_element_past_the_end_is_seen():
    t = gb.guarded((6, 4), torch.float32, "cpu")
    wide = gb.guard_of(t).backing[gb.BAND_BYTES:].view(torch.float32)[:28].view(7, 4)    # the same memory with one more row
    wide[6, 1] = 1.0
    with pytest.raises(gb.GuardViolation) as e:
        gb.check(t)
    assert e.value.side == "back" and 4 <= e.value.offset < 8


def test_allocations_pass_through_for_cpu_and_pinned_and_are_restored():
    before = {n: getattr(torch, n) for n in NAMES}
    with gb.guard_allocations() as net:
        assert all(getattr(torch, n) is not before[n] for n in NAMES)
        a = torch.empty(3, 4)
        b = torch.zeros((3, 4), dtype=torch.float64, device="cpu")
        c = torch.full((2,), 1.5)
        d = torch.empty_like(a)
        e = torch.zeros_like(b, dtype=torch.float32)
        if torch.cuda.is_available():
            p = torch.empty(8, pin_memory=True)
            assert not hasattr(p, "_guard") and p.is_pinned()
        for t in (a, b, c, d, e):
            assert not hasattr(t, "_guard")
        assert b.dtype == torch.float64 and (b == 0).all() and (c == 1.5).all() and e.dtype == torch.float32 and d.shape == a.shape
        assert net.count == 0
    assert all(getattr(torch, n) is before[n] for n in NAMES)


def test_functions_are_restored_after_an_exception():
    before = {n: getattr(torch, n) for n in NAMES}
    with pytest.raises(ZeroDivisionError):
        with gb.guard_allocations():
            assert torch.empty is not before["empty"]
            1 / 0
    assert all(getattr(torch, n) is before[n] for n in NAMES)


def test_interposed_allocations_are_guarded_recorded_and_checked_on_exit():
    """The interposer's device branch without a device: the pass-through test is replaced so that CPU allocations count as device
    allocations."""
    passes = gb._passes_through
    gb._passes_through = lambda device, kwargs, allowed: bool(set(kwargs) - allowed)
    try:
        with gb.guard_allocations() as net:
            a = torch.empty(5, 7)
            b = torch.zeros((5, 7), dtype=torch.int32)
            c = torch.full((3,), 2.5)
            d = torch.full((3,), 7, dtype=torch.int64)
            e = torch.empty_like(a)
            f = torch.zeros_like(a, dtype=torch.float64)
            g = torch.empty((2, 2), dtype=torch.float32, requires_grad=True)
            assert net.count == 7 and all(hasattr(t, "_guard") and t.is_contiguous() for t in (a, b, c, d, e, f, g))
            assert gb.unwritten(a).all() and gb.unwritten(e).all() and (b == 0).all() and (c == 2.5).all() and (d == 7).all() and (f == 0).all()
            assert b.dtype == torch.int32 and d.dtype == torch.int64 and f.dtype == torch.float64 and g.requires_grad
            assert os.path.samefile(gb.guard_of(a).site.rsplit(":", 1)[0], __file__)
        with pytest.raises(gb.GuardViolation) as err:
            with gb.guard_allocations():
                t = torch.empty(4, 4)
                gb.guard_of(t).backing[gb.BAND_BYTES + 64] = 0                   # the byte behind the last element
        assert err.value.side == "back" and err.value.offset == 0
        assert torch.empty is gb._ORIG["empty"]
    finally:
        gb._passes_through = passes
