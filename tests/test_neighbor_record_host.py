"""The checks of the neighbour search's three entries (include/xeq.h: xeq_neighbor_search; csrc/xeq_graph.hip: neighbors_check).  Host
only: it needs the built library and no GPU -- every call below returns before anything is launched, and the pointers it hands over
are host addresses that are never read.  (That the record mirrors the header member for member and has the library's size is
tests/test_resident_records_host.py.)"""
import ctypes
import os
import re

import pytest

from xequinet_amd import lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "xeq.h")
KINDS = ("OPEN_SWEEP", "OPEN_BINS", "PBC_ALL", "PBC_PRUNED", "PBC_BINS")
BIN_KINDS, PERIODIC_KINDS = (lib.NEIGHBORS_OPEN_BINS, lib.NEIGHBORS_PBC_BINS), (lib.NEIGHBORS_PBC_ALL, lib.NEIGHBORS_PBC_PRUNED, lib.NEIGHBORS_PBC_BINS)
POINTERS = "pos ptr img cells shift recip thr lo inv_w nbins bin_base bin_start bin_atom".split()
_SOMEWHERE = (ctypes.c_int64 * 8)()          # a host address for "not NULL"


def _search(kind, n_nodes=7, **members):
    """A record with every pointer set, 27 images and matching reps: complete for any kind."""
    somewhere = ctypes.addressof(_SOMEWHERE)
    rec = lib.fill(lib.NeighborSearch(), dtype=lib.XEQ_F32, kind=kind, n_graphs=1, n_nodes=n_nodes, n_cells=27, cutoff=5.0, reps=(1, 1, 1),
                   **{name: somewhere for name in POINTERS})
    return lib.fill(rec, **members)


def _entries(rec, kinds_with_bins=BIN_KINDS):
    """(entry name, arguments) of the three entries with every output set"""
    out = ctypes.c_void_p(ctypes.addressof(_SOMEWHERE))
    calls = [("xeq_neighbors_count", (rec, out, None)), ("xeq_neighbors_fill", (rec, out, 5, out, out, out, None))]
    if rec.kind in kinds_with_bins:
        calls.insert(0, ("xeq_neighbors_bin_ids", (rec, out, None)))
    return calls


def _null_outputs(name, rec):
    """the entry's arguments with every output NULL"""
    return (rec, None, 5, None, None, None, None) if name == "xeq_neighbors_fill" else (rec, None, None)


def _refused(name, args, *words):
    with pytest.raises(RuntimeError) as err:
        lib.call(name, *args)
    text = str(err.value)
    assert "(1)" in text, text                                       # XEQ_ERR_INVALID_ARGUMENT
    assert text.endswith(lib.load().xeq_last_error().decode())
    for word in (name, *words):
        assert word in text, (word, text)


def test_kinds_are_the_headers():
    text = open(HEADER).read()
    for value, name in enumerate(KINDS):
        assert int(re.search(rf"XEQ_NEIGHBORS_{name}\s*=\s*(\d+)", text).group(1)) == value == getattr(lib, "NEIGHBORS_" + name)
    assert ctypes.sizeof(lib.NeighborSearch) == lib.load().xeq_record_bytes(lib.RECORDS.index(lib.NeighborSearch))


@pytest.mark.parametrize("kind", [-1, 5, 1 << 40])
def test_an_unknown_kind_is_refused(kind):
    for name, args in _entries(_search(kind), kinds_with_bins=(kind,)):
        _refused(name, args, "kind")


@pytest.mark.parametrize("kind", [lib.NEIGHBORS_PBC_PRUNED, lib.NEIGHBORS_PBC_BINS])
@pytest.mark.parametrize("reps", [(1, 1, 0), (2, 1, 1), (-1, 1, 1), (0, 0, 0)])
def test_reps_that_do_not_give_n_cells_are_refused(kind, reps):
    rec = _search(kind, reps=reps)
    for name, args in _entries(rec, kinds_with_bins=()):             # (the bin ids read neither)
        _refused(name, args, "reps", "n_cells")
    if min(reps) >= 0:                                               # ... and accepted with the n_cells they do give
        lib.call("xeq_neighbors_count", _search(kind, reps=reps, n_cells=(2 * reps[0] + 1) * (2 * reps[1] + 1) * (2 * reps[2] + 1), n_nodes=0), None, None)


@pytest.mark.parametrize("kind", BIN_KINDS)
def test_a_bin_grid_fill_without_tmp_keys_is_refused(kind):
    out = ctypes.c_void_p(ctypes.addressof(_SOMEWHERE))
    _refused("xeq_neighbors_fill", (_search(kind), out, 5, None, out, out, None), "tmp_keys")


@pytest.mark.parametrize("kind", PERIODIC_KINDS)
def test_a_periodic_kind_without_img_is_refused(kind):
    for name, args in _entries(_search(kind, img=None), kinds_with_bins=()):
        _refused(name, args, "img")


def test_every_member_a_kind_reads_is_named_when_it_is_missing():
    """Per kind and entry: exactly the members the header lists for it are needed."""
    common, pruned = {"pos", "ptr"}, {"recip", "thr"}
    grid = {"nbins", "bin_base", "bin_start", "bin_atom"}
    reads = {lib.NEIGHBORS_OPEN_SWEEP: common, lib.NEIGHBORS_OPEN_BINS: common | {"lo", "inv_w"} | grid, lib.NEIGHBORS_PBC_ALL: common | {"img"},
             lib.NEIGHBORS_PBC_PRUNED: common | {"img"} | pruned, lib.NEIGHBORS_PBC_BINS: common | {"img"} | pruned | grid}
    for kind, members in reads.items():
        for member in POINTERS:
            for name, args in _entries(_search(kind, **{member: None})):
                needed = member in members
                if name == "xeq_neighbors_fill" and kind in PERIODIC_KINDS and member in ("cells", "shift"):
                    needed = True
                if name == "xeq_neighbors_bin_ids" and member in ("img", "thr", "bin_start", "bin_atom"):
                    needed = False
                if needed:
                    _refused(name, args, f"member {member} ")
                else:
                    with pytest.raises(RuntimeError, match="(rowptr|deg|keys) is NULL"):      # passes the members; refused for its first output
                        lib.call(name, *_null_outputs(name, args[0]))


def test_outputs_and_sizes_are_checked():
    out = ctypes.c_void_p(ctypes.addressof(_SOMEWHERE))
    _refused("xeq_neighbors_count", (_search(lib.NEIGHBORS_OPEN_SWEEP), None, None), "deg")
    _refused("xeq_neighbors_fill", (_search(lib.NEIGHBORS_PBC_ALL), out, 5, None, out, None, None), "cell_offsets")
    _refused("xeq_neighbors_fill", (_search(lib.NEIGHBORS_OPEN_SWEEP), out, -1, None, out, None, None), "n_edges")
    _refused("xeq_neighbors_count", (_search(lib.NEIGHBORS_OPEN_SWEEP, n_graphs=0), out, None), "n_graphs")
    _refused("xeq_neighbors_count", (_search(lib.NEIGHBORS_PBC_ALL, n_cells=0), out, None), "n_cells")
    _refused("xeq_neighbors_count", (_search(lib.NEIGHBORS_OPEN_SWEEP, dtype=2), out, None), "dtype")
    _refused("xeq_neighbors_bin_ids", (_search(lib.NEIGHBORS_PBC_PRUNED), out, None), "no bin grid")
    _refused("xeq_neighbors_count", (None, out, None), "null argument record")


@pytest.mark.parametrize("kind", range(5))
def test_no_nodes_is_no_work_for_every_kind(kind):
    """n_nodes = 0 returns XEQ_OK at once, with NULL everywhere (an empty tensor's address); so does a fill of no edges."""
    empty = lib.fill(lib.NeighborSearch(), dtype=lib.XEQ_F64, kind=kind, n_graphs=0, n_nodes=0, n_cells=1, cutoff=5.0)
    before = lib.launch_count()
    for name, _ in _entries(empty):
        lib.call(name, *_null_outputs(name, empty))
    lib.call("xeq_neighbors_fill", _search(kind), None, 0, None, None, None, None)
    assert lib.launch_count() == before
