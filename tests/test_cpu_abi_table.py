"""_lib.SIGNATURES, the hand-written ctypes table, against include/pointnet_hip.h: arity, return type, every scalar's exact ctypes
type and every pointer's kind, for every entry; and the integer constants _lib.py repeats.  Needs no GPU and does not load the
library.  (Struct layouts are not checked here.)"""
import ctypes as C
import os
import re

from pointcloudprocessing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pointnet_hip.h")

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "uint8_t": C.c_uint8, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "pn_stream": C.c_void_p}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _param(decl):
    """'const float* xyz' -> ('float', True);  'pn_stream stream' -> ('pn_stream', False)"""
    tok = [t for t in re.findall(r"\w+|\*", decl) if t not in ("const", "struct")]
    if "*" in tok:
        return " ".join(tok[:tok.index("*")]), True
    return " ".join(tok[:-1] if len(tok) > 1 else tok), False


def parse_header(path=HEADER):
    """-> ({name: (return type, [(base type, is pointer), ...])}, {PN_* macro: int})"""
    text = _strip_comments(open(path).read()).replace("\\\n", " ")
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(PN_\w+)[ \t]+(\S[^\n]*)$", text, flags=re.M):
        value = re.sub(r"(?<=[0-9a-fA-F])[uUlL]+\b", "", value.strip())
        if re.fullmatch(r"[0-9a-fA-FxX\s()<>+\-*|&~]+", value):
            defines[name] = int(eval(value, {"__builtins__": {}}))
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)                          # preprocessor lines
    text = re.sub(r"typedef\s+(?:struct|enum)[^{;]*\{[^}]*\}\s*\w+\s*;", " ", text)   # type definitions (no nested braces)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\s*\b(pn_\w+)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        args = [] if params in ("", "void") else [_param(p) for p in params.split(",")]
        proto = (_param(ret + " _")[0] + ("*" if "*" in ret else ""), args)
        assert protos.setdefault(name, proto) == proto, f"{name} is declared twice, differently"
    return protos, defines


def _check_type(where, base, pointer, ctype, out):
    if not pointer:
        if base not in SCALARS:
            out.append(f"{where}: the header's type '{base}' is unknown to this test")
        elif ctype is not SCALARS[base]:
            out.append(f"{where}: header {base}, table {getattr(ctype, '__name__', ctype)}")
        return
    if ctype is C.c_void_p:
        return
    if ctype is C.c_char_p:
        if base != "char":
            out.append(f"{where}: c_char_p for {base}*")
        return
    if not (isinstance(ctype, type) and issubclass(ctype, C._Pointer)):
        out.append(f"{where}: header {base}*, table {getattr(ctype, '__name__', ctype)} is no pointer type")
        return
    pointee = ctype._type_
    if issubclass(pointee, C.Structure):
        if pointee.__name__ != base:
            out.append(f"{where}: header {base}*, table POINTER({pointee.__name__})")
    elif base not in SCALARS or pointee is not SCALARS[base]:
        out.append(f"{where}: header {base}*, table POINTER({pointee.__name__})")


def check_table(protos, signatures):
    """every disagreement between the header's prototypes and a SIGNATURES-like table, as text"""
    out = [f"{n}: in the header, not in the table" for n in sorted(set(protos) - set(signatures))]
    out += [f"{n}: in the table, not in the header" for n in sorted(set(signatures) - set(protos))]
    for name in sorted(set(protos) & set(signatures)):
        (ret, params), (restype, argtypes) = protos[name], signatures[name]
        _check_type(f"{name} return", ret.rstrip("*"), ret.endswith("*"), restype, out)
        if len(params) != len(argtypes):
            out.append(f"{name}: header takes {len(params)} arguments, table {len(argtypes)}")
            continue
        for i, ((base, pointer), ctype) in enumerate(zip(params, argtypes)):
            _check_type(f"{name} argument {i}", base, pointer, ctype, out)
    return out


PROTOS, DEFINES = parse_header()


def test_parser_reads_the_header():
    assert len(PROTOS) >= 100 and set(PROTOS) == set(_lib.SIGNATURES)
    assert PROTOS["pn_last_error"] == ("char*", [])
    assert PROTOS["pn_radius_knn_leaf"] == ("float", [("float", False)])
    assert PROTOS["pn_argmax_rows"] == ("int", [("float", True), ("int64_t", False), ("int", False), ("int32_t", True), ("pn_stream", False)])
    assert PROTOS["pn_model_slot_info"][1][2] == ("pn_slot_info", True)
    assert PROTOS["pn_lidar_sense"][1][9:12] == [("uint64_t", False), ("int", False), ("double", False)]


def test_signatures_match_the_header():
    problems = check_table(PROTOS, _lib.SIGNATURES)
    assert problems == [], "\n".join(problems)


def test_constants_match_the_header():
    assert DEFINES["PN_RADIUS_KNN_MAX_KEY"] == 1 << 14 and DEFINES["PN_STORE_BF16"] == 0x100
    assert _lib.ABI_VERSION == DEFINES["PN_ABI_VERSION"]
    shared = [n for n in DEFINES if hasattr(_lib, n)]
    assert "PN_RADIUS_KNN_MAX_KEY" in shared and len(shared) >= 10
    for name in shared:
        assert getattr(_lib, name) == DEFINES[name], f"{name}: header {DEFINES[name]}, _lib.py {getattr(_lib, name)}"


def test_checker_reports_a_swapped_scalar():
    table = dict(_lib.SIGNATURES)
    res, args = table["pn_lidar_sense"]
    i = args.index(C.c_double)
    table["pn_lidar_sense"] = (res, args[:i] + [C.c_float] + args[i + 1:])
    assert check_table(PROTOS, table) == [f"pn_lidar_sense argument {i}: header double, table c_float"]


def test_checker_reports_a_dropped_argument():
    table = dict(_lib.SIGNATURES)
    res, args = table["pn_lidar_sense"]
    table["pn_lidar_sense"] = (res, args[:-1])
    assert check_table(PROTOS, table) == [f"pn_lidar_sense: header takes {len(args)} arguments, table {len(args) - 1}"]
