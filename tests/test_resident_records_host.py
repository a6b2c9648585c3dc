"""The argument records of the resident drivers' entries and of the neighbour search (include/xeq.h: xeq_res_*, xeq_*_params,
xeq_neighbor_search) against their ctypes mirrors in
xequinet_amd/lib.py, and the constants lib.py restates against the header's #define / enum values.  Host only: the header is parsed as
text, the library is asked for its sizes."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "xeq.h")
EIGHT_BYTE_TYPES = {"int64_t", "uint64_t", "double"}          # (and every pointer)


def _header() -> str:
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def _records(text):
    """{name: [(member, is_pointer, base type, array length or 0), ...]} of every ``typedef struct NAME { ... } NAME;``"""
    out = {}
    for name, body, alias in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        assert name == alias, (name, alias)
        members = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+(?:\s*\[\s*\d+\s*\])?(?:\s*,\s*\w+)*)", decl)
            assert m, f"{name}: cannot read the member declaration {decl!r}"
            base, star, names = m.groups()
            for one in names.split(","):
                arr = re.fullmatch(r"\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", one)
                members.append((arr.group(1), bool(star), base, int(arr.group(2) or 0)))
        out[name] = members
    return out


def _constants(text):
    """{NAME: value} of the integer #defines and of the enumerators written ``NAME = value``."""
    out = {k: int(v) for k, v in re.findall(r"^#define\s+(XEQ_\w+)\s+(-?\d+)\s*$", text, flags=re.M)}
    for body in re.findall(r"enum\s*\{(.*?)\}", text, flags=re.S):
        out.update({k: int(v) for k, v in re.findall(r"(XEQ_\w+)\s*=\s*(-?\d+)", body)})
    return out


def test_records_match_the_header_member_for_member():
    from xequinet_amd import lib

    text = _header()
    records, const = _records(text), _constants(text)
    L = lib.load()
    assert sorted(records) == sorted(r.__name__ for r in lib.RECORDS)              # every record of the header has its mirror, and no other
    which = {"xeq_res_system": "SYSTEM", "xeq_res_step": "STEP", "xeq_res_chunks": "CHUNKS", "xeq_res_recorder": "RECORDER", "xeq_md_params": "MD",
             "xeq_npt_params": "NPT", "xeq_fire_params": "FIRE", "xeq_neighbor_search": "NEIGHBORS", "xeq_lbfgs_params": "LBFGS"}
    for index, rec in enumerate(lib.RECORDS):
        members = records[rec.__name__]
        assert const["XEQ_REC_" + which[rec.__name__]] == index, rec.__name__      # lib.RECORDS is in the order of XEQ_REC_*
        assert [f[0] for f in rec._fields_] == [m[0] for m in members], rec.__name__
        for (name, kind), (_, pointer, base, count) in zip(rec._fields_, members):
            assert pointer or base in EIGHT_BYTE_TYPES, (rec.__name__, name, base)                 # 8 bytes in the header ...
            element = kind._type_ if count else kind
            assert ctypes.sizeof(element) == 8 and ctypes.sizeof(kind) == 8 * max(count, 1), (rec.__name__, name)        # ... and in the mirror,
            if not pointer:                                                                         # of the same kind
                assert element is {"int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}[base], (rec.__name__, name)
            else:
                assert element is ctypes.c_void_p, (rec.__name__, name)
        size = 8 * sum(max(m[3], 1) for m in members)
        assert ctypes.sizeof(rec) == size == L.xeq_record_bytes(index), rec.__name__
        assert [getattr(rec, f[0]).offset for f in rec._fields_] == [8 * sum(max(m[3], 1) for m in members[:k]) for k in range(len(members))]
    assert L.xeq_record_bytes(len(lib.RECORDS)) == -1 and L.xeq_record_bytes(-1) == -1
    # the entries take them by pointer
    assert L.xeq_npt_back.argtypes[:6] == [ctypes.POINTER(r) for r in (lib.ResSystem, lib.ResStep, lib.ResChunks, lib.MdParams, lib.NptParams, lib.ResRecorder)]
    assert L.xeq_lbfgs_back.argtypes[:5] == [ctypes.POINTER(r) for r in (lib.ResSystem, lib.ResStep, lib.ResChunks, lib.LbfgsParams, lib.ResRecorder)]


def test_fill_refuses_a_member_the_record_does_not_have():
    import pytest

    from xequinet_amd import lib

    s = lib.fill(lib.ResSystem(), n=3, pos=None)
    assert s.n == 3 and s.pos is None
    with pytest.raises(AttributeError, match="no member 'position'"):
        lib.fill(s, position=1)
    host = (ctypes.c_double * 9)(*range(9))
    assert lib.fill(s, cell=host).cell == ctypes.addressof(host)
    assert list(lib.fill(lib.ResStep(), reps=(1, 2, 3)).reps) == [1, 2, 3]


def test_restated_constants_are_the_headers():
    from xequinet_amd import lib

    const = _constants(_header())
    names = [k for k in const if re.match(r"XEQ_(MD|NPT|FIRE|LBFGS)_", k)]
    assert {"XEQ_MD_CHUNK", "XEQ_MD_NVE", "XEQ_MD_LANGEVIN", "XEQ_MD_BERENDSEN", "XEQ_MD_PURPOSE_LANGEVIN", "XEQ_MD_PURPOSE_MAXWELL", "XEQ_NPT_BOX",
            "XEQ_NPT_CELL", "XEQ_NPT_INV", "XEQ_NPT_CELL_NEXT", "XEQ_NPT_INV_NEXT", "XEQ_NPT_MU", "XEQ_NPT_P", "XEQ_NPT_V", "XEQ_FIRE_FRESH",
            "XEQ_FIRE_ACTIVE", "XEQ_FIRE_CONVERGED", "XEQ_LBFGS_FRESH", "XEQ_LBFGS_ACTIVE", "XEQ_LBFGS_CONVERGED", "XEQ_LBFGS_MAX_MEMORY"} == set(names)
    for k in names:
        assert getattr(lib, k[len("XEQ_"):]) == const[k], k
    from xequinet_amd import md

    assert md.ENSEMBLES == {"nve": const["XEQ_MD_NVE"], "langevin": const["XEQ_MD_LANGEVIN"], "berendsen": const["XEQ_MD_BERENDSEN"],
                            "npt_berendsen": const["XEQ_MD_BERENDSEN"]}
    assert (md.PURPOSE_LANGEVIN, md.PURPOSE_MAXWELL) == (const["XEQ_MD_PURPOSE_LANGEVIN"], const["XEQ_MD_PURPOSE_MAXWELL"])
