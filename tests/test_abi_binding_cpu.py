"""The ctypes binding is derived from include/conformer_hip.h (conformer_amd/_lib.py): these CPU tests pin the derivation.
A second parser written here (a scanner over `cfm_*(` tokens with its own type map, sharing nothing with the product's
regular expression) reads the same header and must agree on every restype and argtype; a few signatures are spelled out in
full against a blind spot both parsers could share; synthetic headers exercise the strictness rules; the constants and the two
hand-written struct mirrors are compared with the header; `_lib.call` is exercised through argument validation, which runs
before any HIP call."""
import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

import pytest

from conformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "conformer_hip.h")

P, I, L, F, D, U, Z = c_void_p, c_int, c_int64, c_float, c_double, c_uint64, c_size_t
SCALARS = {"int": I, "int64_t": L, "float": F, "double": D, "uint64_t": U, "size_t": Z, "cfm_stream_t": P}


def stripped_header() -> str:
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def c_type(text: str, is_return: bool = False):
    """The test's own C type -> ctypes map: `text` is a type with or without a trailing parameter name."""
    words = text.replace("*", " * ").split()
    if "*" in words:
        return c_char_p if is_return and words[:3] == ["const", "char", "*"] else P
    words = [w for w in words if w != "const"]
    if len(words) == 2 and not is_return:           # type + parameter name
        words = words[:1]
    assert len(words) == 1 and words[0] in SCALARS, text
    return SCALARS[words[0]]


def scan_declarations(src: str):
    """name -> (restype, [argtypes]) by scanning: every `cfm_*(` token is a declaration, its return type is the text back to
    the previous `;`, `}` or line of a directive, its parameters run to the next `)`."""
    out = {}
    for m in re.finditer(r"(cfm_\w+)\s*\(", src):
        head = src[:m.start()]
        cut = max(head.rfind(";"), head.rfind("}"), head.rfind("{"))
        ret = head[cut + 1:]
        ret = "\n".join(ln for ln in ret.split("\n") if not ln.lstrip().startswith("#"))
        params = src[m.end():src.index(")", m.end())].strip()
        args = [] if params in ("", "void") else [c_type(a) for a in params.split(",")]
        assert m.group(1) not in out, m.group(1)
        out[m.group(1)] = (c_type(ret, is_return=True), args)
    return out


def struct_fields(src: str, name: str):
    """[(field, ctypes type)] of `typedef struct <name> { ... } <name>;`, one entry per declarator."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), src, flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = [d.strip() for d in decl.split(",")]
        ctype = c_type(first)
        fields.append((first.replace("*", " ").split()[-1], ctype))
        fields += [(d, ctype) for d in more]          # `int64_t rows, cols;`: the later declarators share the first one's type
    return fields


def test_every_type_matches_an_independent_parse():
    mine = scan_declarations(stripped_header())
    assert set(mine) == set(_lib.SIGNATURES)
    assert len(mine) == 144
    for name, (res, args) in mine.items():
        assert _lib.SIGNATURES[name][0] is res, name
        assert _lib.SIGNATURES[name][1] == args, name
        assert len(_lib.PARAMS[name]) == len(args), name


def test_no_declaration_is_skipped():
    assert len(re.findall(r"cfm_\w+\s*\(", stripped_header())) == len(_lib.SIGNATURES)


def test_literal_signatures():
    S = _lib.SIGNATURES
    assert S["cfm_gemm_mfma16_f32"] == (I, [I, I, P, I, P, I, P, P, F, P, I, P, I, L, I, I, L, L, L, F, U, P])
    assert len(S["cfm_gemm_mfma16_f32"][1]) == 22
    assert S["cfm_ctc_beam_lm_decode_f32"] == (I, [P, P, I, I, I, I, I, I, F, F, I, P, D, D, D, I, P, Z, P, P, P, P, P, P])
    assert S["cfm_layernorm_bwd_f32"] == (I, [P, P, P, P, P, P, P, P, P, L, I, P, Z, P])
    assert S["cfm_relpos_attention_slots_mfma16_f32"] == (I, [I, P, P, P, I, L, P, L, P, P, P, P, P, P, L, I, I, I, I, I, I, P, P])
    assert S["cfm_strerror"][0] is c_char_p
    assert S["cfm_ffn_pack_elems"][0] is L
    assert S["cfm_ctc_beam_workspace_bytes"][0] is Z
    assert _lib.PARAMS["cfm_layernorm_fwd_f32"] == ["x", "gamma", "beta", "y", "mean_or_null", "rstd_or_null", "rows", "d", "eps",
                                                    "stream"]


def test_parser_is_strict():
    sigs, params, consts = _lib.parse_header("""
        /* int cfm_in_a_comment(int x); */
        #define CFM_N 7
        int cfm_a(void);
        int64_t cfm_b(int64_t rows, int d);
        const char* cfm_c(
            const float* x,    /* spread over lines */
            double,
            uint64_t seed, size_t n,
            cfm_stream_t stream);
        size_t cfm_d();
    """)
    assert sigs == {"cfm_a": (I, []), "cfm_b": (L, [L, I]), "cfm_c": (c_char_p, [P, D, U, Z, P]), "cfm_d": (Z, [])}
    assert params["cfm_b"] == ["rows", "d"] and params["cfm_c"] == ["x", "arg1", "seed", "n", "stream"]
    assert consts == {"CFM_N": 7}
    with pytest.raises(_lib.ConformerHipError, match="cfm_e"):
        _lib.parse_header("int cfm_e(long double x);")
    with pytest.raises(_lib.ConformerHipError, match="cfm_f"):
        _lib.parse_header("int cfm_a(void);\nlong double cfm_f(int x);")             # unread return type: the count rule
    with pytest.raises(_lib.ConformerHipError, match="cfm_g"):
        _lib.parse_header("unsigned cfm_g(int x);")
    with pytest.raises(_lib.ConformerHipError):
        _lib.parse_header("int cfm_a(void); int cfm_h(void);")                       # the second one is not at a line's start


def test_constants_come_from_the_header():
    from conformer_amd import align, ops
    src = stripped_header()
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(CFM_\w+)\s+(-?\d+)", src)}
    assert defines == {"CFM_ABI_VERSION": 4, "CFM_PREC_F32": 0, "CFM_PREC_BF16": 1, "CFM_PREC_FP16": 2, "CFM_CAST_BATCH": 48,
                       "CFM_CTC_MAX_TARGET": 1023, "CFM_CTC_ALIGN_MAX_FRAMES": 16384, "CFM_CTC_ALIGN_MAX_TARGET": 4096,
                       "CFM_CTC_ALIGN_WAVE_MAX_TARGET": 1023}
    status = {"CFM_OK": 0, "CFM_ERR_BAD_SHAPE": -1, "CFM_ERR_UNSUPPORTED": -2, "CFM_ERR_NULL": -3, "CFM_ERR_LAUNCH": -4,
              "CFM_ERR_DEVICE": -5, "CFM_ERR_ALIGN": -6}
    body = src[src.index("enum cfm_status"):]
    assert {k: int(v) for k, v in re.findall(r"(CFM_\w+)\s*=\s*(-?\d+)", body[:body.index("}")])} == status
    assert _lib.CONSTANTS == {**defines, **status}
    assert _lib.ABI_VERSION == 4
    assert (ops.PREC_F32, ops.PREC_BF16, ops.PREC_FP16) == (0, 1, 2)
    assert ops.CTC_MAX_TARGET == 1023 and align.MAX_FRAMES == 16384 and align.MAX_TARGET == 4096


def test_struct_mirrors_match_the_header():
    from conformer_amd import optim
    src = stripped_header()
    cast = struct_fields(src, "cfm_cast_item")
    assert cast == [("src", P), ("dst", P), ("rows", L), ("cols", L), ("transpose", I)]
    assert list(_lib.CastItem._fields_) == cast
    adam = struct_fields(src, "cfm_adam_tensor")
    assert adam == [("param", P), ("grad", P), ("exp_avg", P), ("exp_avg_sq", P), ("numel", L)]
    assert list(optim._AdamTensor._fields_) == adam
    assert ctypes.sizeof(_lib.CastItem) == 40 and ctypes.sizeof(optim._AdamTensor) == 40


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_call_raises_with_the_entry_name_and_counts_once(lib):
    null_text = lib.cfm_strerror(-3).decode()
    before = _lib.CALLS[0]
    with pytest.raises(_lib.ConformerHipError) as e:
        _lib.call("cfm_layernorm_fwd_f32", None, None, None, None, None, None, 4, 32, 1e-5, None)
    assert str(e.value) == f"cfm_layernorm_fwd_f32 failed: {null_text} (status -3)"
    assert _lib.CALLS[0] == before + 1
    buf = (ctypes.c_float * 4096)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    args = [a, 512, a, 16, 1e-5, a, a, a, a, 0.5, a, 512, 0, None, None, None, 0.0, 0, 512, 2048, None]      # M = 0: no launch
    assert _lib.call("cfm_ffn_fused_f32", *args) is None
    assert _lib.CALLS[0] == before + 2


def test_call_looks_the_entry_up_at_call_time(lib):
    real, seen = lib.cfm_layernorm_fwd_f32, []
    before = _lib.CALLS[0]
    try:
        lib.cfm_layernorm_fwd_f32 = lambda *a: seen.append(a) or 0
        _lib.call("cfm_layernorm_fwd_f32", 1, 2, 3)
        lib.cfm_layernorm_fwd_f32 = lambda *a: seen.append(a) or -2
        with pytest.raises(_lib.ConformerHipError, match=r"cfm_layernorm_fwd_f32 failed: .* \(status -2\)"):
            _lib.call("cfm_layernorm_fwd_f32", 4)
    finally:
        lib.cfm_layernorm_fwd_f32 = real
    assert seen == [(1, 2, 3), (4,)] and _lib.CALLS[0] == before + 2
    assert lib.cfm_layernorm_fwd_f32(None, None, None, None, None, None, 4, 32, 1e-5, None) == -3


def test_call_names_the_parameter_of_a_wrong_python_type(lib):
    before = _lib.CALLS[0]
    with pytest.raises(_lib.ConformerHipError) as e:
        _lib.call("cfm_layernorm_fwd_f32", None, None, None, None, None, None, "4", 32, 1e-5, None)
    assert "cfm_layernorm_fwd_f32" in str(e.value) and "`rows`" in str(e.value)
    assert _lib.CALLS[0] == before + 1
