"""The ctypes mirror (optical_networking_gym/_native.py) held to include/ongym.h without loading the library: every prototype
against its row of SIGNATURES argument by argument, the six structs declarator by declarator, every enumerator and numeric
#define against its Python name.  The comparison functions take the parsed header and the Python side as arguments and return
the list of disagreements; the last tests hand them doctored copies of the Python side and expect each one to be named."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from optical_networking_gym import _native as nat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = open(os.path.join(REPO, "include", "ongym.h")).read()
TEXT = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", RAW, flags=re.S))      # comments stripped

SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "float": C.c_float, "double": C.c_double}
RETURNS = {"int": C.c_int32, "int32_t": C.c_int32, "void": None, "double": C.c_double, "const char *": C.c_char_p}
NUMPY = {"float": "<f4", "double": "<f8", "int16_t": "<i2", "int32_t": "<i4", "int64_t": "<i8", "uint8_t": "u1"}
DTYPES = {"ongym_request": nat.REQUEST_DTYPE, "ongym_step_rec": nat.STEP_DTYPE, "ongym_service": nat.SERVICE_DTYPE,
          "ongym_move": nat.MOVE_DTYPE, "ongym_stats": nat.STATS_DTYPE}
STRUCTS = {"ongym_config": nat.OngymConfig}


# ---- the header, parsed ------------------------------------------------------------------------------------------------------
def _declarator(base, text):
    """(name, base type, pointer depth, array length or None) of one declarator `**name[n]`"""
    m = re.fullmatch(r"(\**)\s*(\w+)\s*(?:\[(\d+)\])?", text.strip())
    assert m, (base, text)
    return m.group(2), base, len(m.group(1)), int(m.group(3)) if m.group(3) else None


def _declaration(text):
    """the declarators of `[const] type a, *b, c[8]`"""
    m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(.*)", " ".join(text.split()))
    assert m, text
    return [_declarator(m.group(1), d) for d in m.group(2).split(",")]


def parse_prototypes(text):
    """[(name, return type, [(name, base, pointer depth, array length)])] in the header's order"""
    body = re.sub(r"typedef struct \w+ \{.*?\} \w+;", "", text, flags=re.S)
    body = re.sub(r"enum \{.*?\};", "", body, flags=re.S)
    out = []
    for ret, name, params in re.findall(r"^([A-Za-z_][\w \*]*?)\b(ongym_\w+)\s*\(([^)]*)\)\s*;", body, flags=re.M):
        params = " ".join(params.split())
        args = [] if params in ("", "void") else [_declaration(p)[0] for p in params.split(",")]
        out.append((name, " ".join(ret.split()), args))
    return out


def parse_structs(text):
    """{struct: [(name, base, pointer depth, array length)]} of every `typedef struct X { ... } X;`"""
    out = {}
    for tag, body, name in re.findall(r"typedef struct (\w+) \{(.*?)\} (\w+);", text, flags=re.S):
        assert tag == name
        out[name] = [d for stmt in body.split(";") if stmt.strip() for d in _declaration(stmt)]
    return out


def parse_constants(text):
    """{name: value} of every enumerator and every #define with an integer value"""
    out = {}
    for body in re.findall(r"enum \{(.*?)\};", text, flags=re.S):
        value = -1
        for item in filter(None, (" ".join(i.split()) for i in body.split(","))):
            name, _, given = item.partition(" = ")
            value = int(given, 0) if given else value + 1
            assert re.fullmatch(r"ONGYM_\w+", name) and name not in out, item
            out[name] = value
    for name, given in re.findall(r"^#define (ONGYM_\w+)[ \t]+(-?\w+)[ \t]*$", text, flags=re.M):
        assert name not in out
        out[name] = int(given, 0)
    return out


def parse_sizeof_order(raw):
    """the struct of every index of ongym_sizeof, from the comment at its prototype"""
    m = re.search(r"ongym_sizeof\(int32_t what\);\s*/\*(.*?)\*/", raw)
    pairs = re.findall(r"(\d+) (\w+)", m.group(1))
    assert [int(i) for i, _ in pairs] == list(range(len(pairs)))
    return ["ongym_" + word for _, word in pairs]


PROTOTYPES, HEADER_STRUCTS, CONSTANTS = parse_prototypes(TEXT), parse_structs(TEXT), parse_constants(TEXT)


# ---- the comparisons: (header, Python side) -> the list of disagreements -----------------------------------------------------
def _argument_problem(decl, ctype, structs):
    """None, or why `ctype` does not carry the parameter `decl`"""
    _, base, depth, array = decl
    depth += array is not None
    if depth == 0:
        return None if ctype is SCALARS.get(base, ()) else f"header {base}, python {getattr(ctype, '__name__', ctype)}"
    if ctype is C.c_void_p:
        return None
    if not (isinstance(ctype, type) and issubclass(ctype, C._Pointer)):
        return f"header {base} {'*' * depth}, python {getattr(ctype, '__name__', ctype)}"
    want = C.c_void_p if depth == 2 else SCALARS.get(base, structs.get(base, ()))
    return None if ctype._type_ is want else f"header {base} {'*' * depth}, python POINTER({ctype._type_.__name__})"


def prototype_problems(prototypes, signatures, structs):
    out = []
    if [p[0] for p in prototypes] != list(signatures):
        out.append(f"order or set of functions: header only {[p[0] for p in prototypes if p[0] not in signatures]}, python only "
                   f"{[n for n in signatures if n not in {p[0] for p in prototypes}]}, or another order")
    for name, ret, args in prototypes:
        if name not in signatures:
            continue
        restype, argtypes = signatures[name]
        if ret not in RETURNS or restype is not RETURNS[ret]:
            out.append(f"{name}: returns {ret}, python {getattr(restype, '__name__', restype)}")
        if len(args) != len(argtypes):
            out.append(f"{name}: {len(args)} parameters, python {len(argtypes)}")
            continue
        for i, (decl, ctype) in enumerate(zip(args, argtypes)):
            why = _argument_problem(decl, ctype, structs)
            if why:
                out.append(f"{name}: parameter {i} ({decl[0]}): {why}")
    return out


def config_problems(fields, ctypes_fields):
    """ongym_config against OngymConfig._fields_: name, order and type of every field"""
    out = []
    if len(fields) != len(ctypes_fields):
        out.append(f"ongym_config: {len(fields)} fields, python {len(ctypes_fields)}")
    for (name, base, depth, array), (py_name, ctype) in zip(fields, ctypes_fields):
        want = SCALARS.get(base) if depth == 0 else C.POINTER(SCALARS[base]) if depth == 1 else None
        if name != py_name or array is not None or want is None or ctype is not want:
            out.append(f"ongym_config.{name}: header {base} {'*' * depth}, python {py_name} {ctype.__name__}")
    return out


def header_dtype(fields):
    """the numpy dtype that lays a header struct out as the C compiler does"""
    assert all(depth == 0 for _, _, depth, _ in fields)
    return np.dtype([(name, NUMPY[base]) + (((array,),) if array else ()) for name, base, _, array in fields], align=True)


def record_problems(struct, fields, dtype):
    """a header struct against its numpy dtype: name, order, type, shape and offset of every field, then the size"""
    want, out = header_dtype(fields), []
    if len(want.names) != len(dtype.names):
        out.append(f"{struct}: {len(want.names)} fields, python {len(dtype.names)}")
    for a, b in zip(want.names, dtype.names):
        if a != b or want.fields[a][:2] != dtype.fields[b][:2]:
            out.append(f"{struct}.{a}: header {want.fields[a][:2]}, python {b} {dtype.fields[b][:2]}")
    if not out and (want != dtype or want.itemsize != dtype.itemsize):
        out.append(f"{struct}: header {want.itemsize} bytes, python {dtype.itemsize}")
    return out


def constant_problems(constants, namespace):
    """every ONGYM_<NAME> against namespace[<NAME>]; an ONGYM_N_<X> counts the names of the column tuple namespace[<X>]"""
    out = []
    for name, value in constants.items():
        short = name[len("ONGYM_"):]
        if short.startswith("N_"):
            got = len(namespace[short[2:]]) if isinstance(namespace.get(short[2:]), tuple) else None
        else:
            got = namespace.get(short)
        if type(got) is not int or got != value:
            out.append(f"{name}: header {value}, python {got}")
    return out


# ---- header and mirror agree -------------------------------------------------------------------------------------------------
def test_prototypes_equal_signatures_in_order_and_type():
    names = [p[0] for p in PROTOTYPES]
    assert len(names) == len(set(names)) == 55
    assert set(names) == set(re.findall(r"\b(ongym_[a-z_]+)\s*\(", RAW))       # test_library_exports_every_declared_symbol's
    assert names == list(nat.SIGNATURES) == list(nat.EXPORTED_SYMBOLS)
    assert prototype_problems(PROTOTYPES, nat.SIGNATURES, STRUCTS) == []
    assert set(nat.ABSENT_FROM_OLDER_BUILDS) < set(names) and len(set(nat.ABSENT_FROM_OLDER_BUILDS)) == 15


def test_structs_equal_their_mirrors_declarator_by_declarator():
    assert list(HEADER_STRUCTS) == ["ongym_config", "ongym_request", "ongym_step_rec", "ongym_service", "ongym_move", "ongym_stats"]
    assert len(HEADER_STRUCTS["ongym_config"]) == 49
    assert config_problems(HEADER_STRUCTS["ongym_config"], nat.OngymConfig._fields_) == []
    for struct, dtype in DTYPES.items():
        assert record_problems(struct, HEADER_STRUCTS[struct], dtype) == []
        assert header_dtype(HEADER_STRUCTS[struct]) == dtype
    assert [DTYPES[s].itemsize for s in ("ongym_request", "ongym_step_rec", "ongym_service", "ongym_move", "ongym_stats")] \
        == [16, 56, 32, 32, 440]


def test_load_library_expects_the_size_of_the_struct_ongym_sizeof_names():
    order = parse_sizeof_order(RAW)
    assert order == [struct for struct, _ in nat.STRUCT_SIZES] and sorted(order) == sorted(HEADER_STRUCTS)
    for struct, size in nat.STRUCT_SIZES:
        expect = C.sizeof(nat.OngymConfig) if struct == "ongym_config" else header_dtype(HEADER_STRUCTS[struct]).itemsize
        assert size == expect, struct


def test_every_constant_of_the_header_has_its_python_name():
    assert len(CONSTANTS) >= 40 + 14 + 15 and CONSTANTS["ONGYM_ABI_VERSION"] == nat.ABI_VERSION == 4
    assert constant_problems(CONSTANTS, vars(nat)) == []
    counts = {name[len("ONGYM_N_"):]: value for name, value in CONSTANTS.items() if name.startswith("ONGYM_N_")}
    assert counts == {"LINK_METRICS": 8, "LINK_STATS": 4, "SERVICE_QOT": 4, "REPLICA_QOT": 6, "LINK_QOT": 3, "ACTION_IMPACT": 8,
                      "FAILURE_IMPACT": 10, "FAILURE_SETS": 12, "CUT_LINKS": 13, "MOVE_COLUMNS": 6, "SPECTRUM_AUDIT_COLUMNS": 10,
                      "SPECTRUM_RECORD_COLUMNS": 6, "ADMISSION_MAP": 8, "PLAYOUT": 8}
    for tuple_name, count in counts.items():
        assert len(getattr(nat, tuple_name)) == count, tuple_name


# ---- not vacuous: a doctored Python side is reported, with the function or field named ---------------------------------------
def _row(name, restype=..., drop_last=False, **replace):
    """SIGNATURES with one row changed: its restype, its last argument dropped, or argument `argN` replaced"""
    ret, args = nat.SIGNATURES[name]
    args = list(args[:-1] if drop_last else args)
    for key, ctype in replace.items():
        args[int(key[3:])] = ctype
    return dict(nat.SIGNATURES, **{name: (ret if restype is ... else restype, tuple(args))})


@pytest.mark.parametrize("signatures, named", [
    (_row("ongym_playout", drop_last=True), "ongym_playout: 9 parameters, python 8"),
    (_row("ongym_playout", arg6=C.c_int32), "ongym_playout: parameter 6 (seed): header uint64_t, python c_int"),
    (_row("ongym_seed_base", arg2=C.c_int32), "ongym_seed_base: parameter 2 (replica_base): header uint64_t, python c_int"),
    (_row("ongym_reset", arg1=C.c_int32), "ongym_reset: parameter 1 (mask): header uint8_t *, python c_int"),
    (_row("ongym_query_gsnr", arg5=C.c_double), "ongym_query_gsnr: parameter 5 (out): header double *, python c_double"),
    (_row("ongym_state_size", arg2=C.POINTER(C.c_int32)), "ongym_state_size: parameter 2 (bytes): header int64_t *, python POINTER(c_int)"),
    (_row("ongym_last_kernel_ms", restype=C.c_int32), "ongym_last_kernel_ms: returns double, python c_int"),
    (_row("ongym_destroy", restype=C.c_int32), "ongym_destroy: returns void, python c_int"),
    (_row("ongym_last_error", restype=C.c_void_p), "ongym_last_error: returns const char *, python c_void_p"),
], ids=["one-argument-fewer", "int32-for-uint64", "int32-for-uint64-base", "scalar-for-pointer", "scalar-for-array",
        "wrong-pointee", "wrong-restype", "restype-for-void", "restype-for-string"])
def test_a_doctored_row_is_reported_with_its_function(signatures, named):
    assert prototype_problems(PROTOTYPES, signatures, STRUCTS) == [named]


def test_a_missing_or_misplaced_row_is_reported():
    fewer = {k: v for k, v in nat.SIGNATURES.items() if k != "ongym_gae"}
    assert any("ongym_gae" in p for p in prototype_problems(PROTOTYPES, fewer, STRUCTS))
    moved = dict(reversed(list(nat.SIGNATURES.items())))
    assert len(prototype_problems(PROTOTYPES, moved, STRUCTS)) == 1


def _stats(change):
    """STATS_DTYPE rebuilt from its field list after change(list of [name, format, shape])"""
    fields = [[n, nat.STATS_DTYPE.fields[n][0].base.str, nat.STATS_DTYPE.fields[n][0].shape] for n in nat.STATS_DTYPE.names]
    change(fields)
    return np.dtype([tuple(f) for f in fields], align=True)


def _swap(fields):
    i = [f[0] for f in fields].index("episode_defrag_cycles")
    assert fields[i + 1][0] == "episode_service_reallocations" and fields[i][1:] == fields[i + 1][1:]
    fields[i], fields[i + 1] = fields[i + 1], fields[i]


def _short_hist(fields):
    next(f for f in fields if f[0] == "episode_modulation_hist")[2] = (7,)


def test_doctored_structs_are_reported_with_their_field():
    assert _stats(lambda fields: None) == nat.STATS_DTYPE
    swapped = _stats(_swap)
    assert swapped.itemsize == nat.STATS_DTYPE.itemsize            # what the size check of load_library cannot see
    got = record_problems("ongym_stats", HEADER_STRUCTS["ongym_stats"], swapped)
    assert len(got) == 2 and got[0].startswith("ongym_stats.episode_defrag_cycles:") \
        and got[1].startswith("ongym_stats.episode_service_reallocations:")
    got = record_problems("ongym_stats", HEADER_STRUCTS["ongym_stats"], _stats(_short_hist))
    assert got and got[0].startswith("ongym_stats.episode_modulation_hist:") and "(7,)" in got[0]
    fields = list(nat.OngymConfig._fields_)
    i = [n for n, _ in fields].index("replica_load")
    fields[i], fields[i + 1] = fields[i + 1], fields[i]             # two pointers of one type
    got = config_problems(HEADER_STRUCTS["ongym_config"], fields)
    assert len(got) == 2 and got[0].startswith("ongym_config.replica_load:") and got[1].startswith("ongym_config.replica_margin:")
    fields = list(nat.OngymConfig._fields_)
    fields[[n for n, _ in fields].index("mod_se")] = ("mod_se", C.POINTER(C.c_double))
    assert config_problems(HEADER_STRUCTS["ongym_config"], fields) == ["ongym_config.mod_se: header int32_t *, python mod_se LP_c_double"]


@pytest.mark.parametrize("name, value, named", [
    ("F_QOT_ERROR", nat.F_QOT_ERROR + 1, "ONGYM_F_QOT_ERROR: header 4, python 5"),
    ("E_LIMIT", nat.E_LIMIT + 1, "ONGYM_E_LIMIT: header -5, python -4"),
    ("MAX_OWNER_CAPACITY", nat.MAX_OWNER_CAPACITY + 1, "ONGYM_MAX_OWNER_CAPACITY: header 32766, python 32767"),
    ("MOVE_LOG", None, "ONGYM_MOVE_LOG: header 64, python None"),
    ("PLAYOUT", nat.PLAYOUT[:-1], "ONGYM_N_PLAYOUT: header 8, python 7"),
    ("CUT_LINKS", nat.CUT_LINKS[:-1], "ONGYM_N_CUT_LINKS: header 13, python 12"),
], ids=["enumerator-off-by-one", "error-code-off-by-one", "limit-off-by-one", "no-mirror", "tuple-one-short", "cut-tuple-one-short"])
def test_a_doctored_constant_is_reported_with_its_name(name, value, named):
    namespace = dict(vars(nat), **{name: value})
    if value is None:
        del namespace[name]
    assert constant_problems(CONSTANTS, namespace) == [named]
