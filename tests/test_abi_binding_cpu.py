"""The ctypes binding is derived from the headers under include/ (conformer_amd/_lib.py): these CPU tests pin the derivation.
A second parser written here (a scanner over `cfm_*(` tokens with its own type map, sharing nothing with the product's
regular expression) reads the same headers and must agree on every restype and argtype; a few signatures are spelled out in
full against a blind spot both parsers could share; synthetic headers exercise the strictness rules; the constants and the two
hand-written struct mirrors are compared with the header; `_lib.call` is exercised through argument validation, which runs
before any HIP call.  The last section holds, once for every header, what each entry family used to restate for its own: the
record is the parse of the file, the names are the ones listed here, the library binds them as declared, a library without
them asks for a rebuild, and the build and the build hook follow the table."""
import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

import pytest

from conformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "conformer_hip.h")

P, I, L, F, D, U, Z = c_void_p, c_int, c_int64, c_float, c_double, c_uint64, c_size_t
SCALARS = {"int": I, "int64_t": L, "float": F, "double": D, "uint64_t": U, "size_t": Z, "cfm_stream_t": P}


def stripped_header(path: str = HEADER) -> str:
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


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
    """every header of include/ (listed here, not taken from the binding's table), all 162 entries"""
    mine = {}
    for basename in sorted(os.listdir(INCLUDE)):
        found = scan_declarations(stripped_header(os.path.join(INCLUDE, basename)))
        assert set(found) == set(_lib.HEADERS[basename].signatures), basename
        assert not set(found) & set(mine), basename
        mine.update(found)
    assert set(mine) == set(_lib.ENTRIES)
    assert len(mine) == 162 and len(scan_declarations(stripped_header())) == len(_lib.SIGNATURES) == 144
    for name, (res, args) in mine.items():
        assert _lib.ENTRIES[name][0] is res, name
        assert _lib.ENTRIES[name][1] == args, name
        assert len(_lib.PARAMS[name]) == len(args), name


def test_no_declaration_is_skipped():
    assert len(re.findall(r"cfm_\w+\s*\(", stripped_header())) == len(_lib.SIGNATURES)
    for header in _lib.HEADERS.values():
        assert len(re.findall(r"cfm_\w+\s*\(", stripped_header(header.path))) == len(header.signatures), header.path


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


# ---- every header of include/: one table in the binding, and the build and the hook follow it ----------------------------------
# the entries of each header in the order it declares them, the headers in the order they were added
NAMES = {
    "conformer_hip.h": """
        cfm_version cfm_abi_version cfm_strerror cfm_device_check cfm_layernorm_fwd_f32 cfm_gemm_bias_f32 cfm_gemm_bias_swish_f32
        cfm_gemm_bias_relu_f32 cfm_gemm_bias_glu_f32 cfm_gemm_bias_residual_f32 cfm_gemm_splitk_f32 cfm_gemm_bias_stats_f32
        cfm_gemm_bias_residual_stats_f32 cfm_gemm_lnfold_f32 cfm_layernorm_fwd_stats_f32 cfm_ffn_pack_elems cfm_ffn_pack_f32
        cfm_ffn_fused_f32 cfm_rowgemm_pack_f32 cfm_rowchain_f32 cfm_ffn_tile_stride_f4 cfm_ffn_rotate cfm_relpos_table_f32
        cfm_relpos_attention_fwd_f32 cfm_dwconv_bn_swish_fwd_f32 cfm_convmod_glu_dwconv_f32 cfm_subsample_conv1_relu_f32
        cfm_pack_conv2_weight_f32 cfm_subsample_conv2_relu_f32 cfm_pack_linear_weight_f32 cfm_conv2_wino_plane_elems
        cfm_pack_conv2_wino_weight_f32 cfm_subsample_conv2_wino_relu_f32 cfm_gemm_mfma16_f32 cfm_cast16_multi_f32
        cfm_layernorm_fwd_out16_f32 cfm_cast16_f32 cfm_relpos_attention_mfma16_f32 cfm_relpos_attention_rows_mfma16_f32
        cfm_relpos_attention_io16_mfma16_f32 cfm_subsample_conv2_relu_mfma16_f32 cfm_subsample_conv1_relu_out16_f32
        cfm_gemm_bwd_batched_mfma16_f32 cfm_linear_bwd_weight_mfma16_f32 cfm_subsample_conv2_rowtab_elems
        cfm_subsample_conv2_bwd_weight_h16_mfma16_f32 cfm_dwconv_bn_swish_fwd_out16_f32 cfm_glu_bwd_out16_f32 cfm_relu_bwd_out16_f32
        cfm_subsample_conv2_bwd_input_fwdkernel_mfma16_f32 cfm_subsample_conv2_bwd_input_fwdkernel_out16_mfma16_f32
        cfm_subsample_conv1_bwd_d16_f32 cfm_subsample_conv2_bwd_weight_mfma16_f32 cfm_subsample_conv2_bwd_input_mfma16_f32
        cfm_reflect_pad_f32 cfm_power_mel_log_f32 cfm_power_mel_log_mfma_f32 cfm_dft_frames_f32 cfm_specaugment_apply_f32
        cfm_gemm_bias_swish_save_f32 cfm_gemm_bwd_f32 cfm_gemm_bwd_batched_f32 cfm_gemm_train_f32 cfm_relpos_attention_train_f32
        cfm_dropout_f32 cfm_dropout_out16_f32 cfm_layernorm_bwd_dx_f32 cfm_layernorm_bwd_params_f32
        cfm_layernorm_bwd_workspace_bytes cfm_layernorm_bwd_f32 cfm_colsum_f32 cfm_glu_fwd_f32 cfm_glu_bwd_f32
        cfm_dwconv_bn_swish_bwd_f32 cfm_dwconv_bn_stats_workspace_bytes cfm_dwconv_bn_stats_f32 cfm_relpos_attention_bwd_f32
        cfm_relpos_attention_bwd_mfma16_f32 cfm_debug_attention_bwd_trace_f32 cfm_debug_attention_bwd_trace_mfma16
        cfm_debug_dw16_trace cfm_debug_lstm_trace cfm_debug_gemm_mfma16_force_tile cfm_debug_gemm_mfma16_trace
        cfm_debug_gemm_last_tile cfm_debug_gemm_cfg_f32 cfm_debug_ffn_trace cfm_debug_ffn_variant cfm_debug_convmod_variant
        cfm_debug_ffn_layout cfm_debug_set_conv2_bk cfm_relu_bwd_f32 cfm_subsample_conv2_bwd_weight_f32 cfm_pack_conv2_weight_t_f32
        cfm_subsample_conv2_bwd_input_f32 cfm_subsample_conv1_bwd_f32 cfm_adam_step_f32 cfm_greedy_ctc_decode_f32
        cfm_ctc_beam_workspace_bytes cfm_ctc_beam_decode_f32 cfm_ngram_lm_pack_bytes cfm_ngram_lm_pack cfm_ngram_lm_score_f64
        cfm_ctc_beam_lm_workspace_bytes cfm_ctc_beam_lm_decode_f32 cfm_hotword_pack_bytes cfm_hotword_pack cfm_hotword_count
        cfm_ctc_beam_hw_workspace_bytes cfm_ctc_beam_hw_decode_f32 cfm_ctc_beam_stream_state_bytes cfm_ctc_beam_stream_init
        cfm_ctc_beam_stream_step_f32 cfm_ctc_beam_stream_finish_f32 cfm_ctc_beam_stream_reset_slots cfm_lstm_fwd_f32
        cfm_lstm_bwd_f32 cfm_lstm_fwd_frag_f32 cfm_lstm_bwd_frag_f32 cfm_lstm_fwd_mfma16_f32 cfm_lstm_fwd_carry_f32
        cfm_lstm_fwd_frag_carry_f32 cfm_lstm_fwd_mfma16_carry_f32 cfm_lstm_bwd_mfma16_f32 cfm_swish_bn_eval_f32
        cfm_swish_bn_stats_f32 cfm_swish_bn_bwd_f32 cfm_split_pack_elems cfm_split_pack_bf16_f32 cfm_gemm_split_bf16_f32
        cfm_subsample_conv2_relu_split_bf16_f32 cfm_ctc_workspace_floats cfm_ctc_loss_fwd_f32 cfm_ctc_loss_bwd_f32
        cfm_ctc_align_workspace_bytes cfm_ctc_align_f32 cfm_relpos_attention_rows_f32 cfm_relpos_attention_slots_f32
        cfm_relpos_attention_slots_mfma16_f32 cfm_debug_attention_trace_f32 cfm_debug_set_attention_waves cfm_debug_set_bwd_tile
        cfm_subsampled_length cfm_subsampled_lengths_i64""".split(),
    "conformer_hip_window.h": ["cfm_relpos_attention_window_f32"],
    "conformer_hip_commit.h": ["cfm_ctc_beam_commit_state_bytes", "cfm_ctc_beam_stream_commit", "cfm_ctc_beam_commit_reset_slots"],
    "conformer_hip_times.h": ["cfm_ctc_beam_times_bytes", "cfm_ctc_beam_times_reset", "cfm_ctc_beam_stream_step_times_f32",
                              "cfm_ctc_beam_stream_finish_times_f32", "cfm_ctc_beam_stream_commit_times"],
    "conformer_hip_stream_frontend.h": ["cfm_stream_stage_f32"],
    "conformer_hip_resample.h": ["cfm_resample_f32", "cfm_resample_i16"],
    "conformer_hip_endpoint.h": ["cfm_endpoint_step_f32"],
    "conformer_hip_error_rate.h": ["cfm_error_rate_units", "cfm_error_rate_distance"],
    "conformer_hip_confidence.h": ["cfm_confidence_frames_f32", "cfm_confidence_spans_f32", "cfm_confidence_greedy_spans_i64"],
}
BASENAMES = list(NAMES)


def test_the_table_names_every_header_of_include():
    assert sorted(os.listdir(INCLUDE)) == sorted(NAMES)                   # a header nobody registered fails here
    assert list(_lib.HEADERS) == BASENAMES and BASENAMES[0] == "conformer_hip.h" == os.path.basename(_lib.HEADER_PATH)
    assert _lib.HEADERS["conformer_hip.h"].signatures is _lib.SIGNATURES
    assert _lib.HEADERS["conformer_hip.h"].constants is _lib.CONSTANTS
    assert [len(names) for names in NAMES.values()] == [144, 1, 3, 5, 1, 2, 1, 2, 3]


def test_no_name_is_declared_in_two_headers():
    names = [name for header in _lib.HEADERS.values() for name in header.signatures]
    assert len(names) == len(set(names)) == 162
    assert list(_lib.ENTRIES) == names == [name for listed in NAMES.values() for name in listed]
    assert set(_lib.PARAMS) == set(names)


@pytest.mark.parametrize("basename", BASENAMES)
def test_a_header_record_is_the_parse_of_its_file(basename):
    header = _lib.HEADERS[basename]
    assert header.path == os.path.join(INCLUDE, basename)
    with open(header.path) as f:
        text = f.read()
    assert _lib.parse_header(text) == (header.signatures, header.params, header.constants)
    assert list(header.signatures) == NAMES[basename]
    for name, sig in header.signatures.items():
        assert _lib.ENTRIES[name] == sig and _lib.PARAMS[name] == header.params[name], name
        assert len(header.params[name]) == len(sig[1]), name
        assert _lib.header_of(name) == basename
    if basename not in ("conformer_hip.h", "conformer_hip_confidence.h"):
        assert header.constants == {} and "#define CFM_" not in text      # no CFM_* constant of its own


def test_confidence_constants_stay_with_their_header():
    constants = _lib.HEADERS["conformer_hip_confidence.h"].constants
    assert constants == {"CFM_CONFIDENCE_MAX_PROB": 0, "CFM_CONFIDENCE_ENTROPY": 1, "CFM_CONFIDENCE_TSALLIS": 2,
                         "CFM_CONFIDENCE_RENYI": 3, "CFM_CONFIDENCE_MEAN": 0, "CFM_CONFIDENCE_MIN": 1, "CFM_CONFIDENCE_MAX": 2,
                         "CFM_CONFIDENCE_PROD": 3}
    assert not set(constants) & set(_lib.CONSTANTS)


def test_declared_equals_defined():
    """`_lib.call` looks a name up on the CDLL: an exported entry that no header declares would be called with ctypes' default
    conversions.  A source scan, no library needed."""
    csrc = os.path.join(ROOT, "conformer_amd", "csrc")
    defined = []
    for f in sorted(os.listdir(csrc)):
        if f.endswith(".hip"):
            defined += re.findall(r'extern\s+"C"[^;{()]*?\b(cfm_\w+)\s*\([^()]*\)\s*\{', open(os.path.join(csrc, f)).read())
    assert len(defined) == len(set(defined)) == 162
    assert set(defined) == set(_lib.ENTRIES), set(defined) ^ set(_lib.ENTRIES)


def test_every_call_literal_names_an_entry():
    called = set()
    for dp, _, files in os.walk(os.path.join(ROOT, "conformer_amd")):
        for f in files:
            if f.endswith(".py"):
                called |= set(re.findall(r'_lib\.call\(\s*"(cfm_\w+)"', open(os.path.join(dp, f)).read()))
    assert len(called) > 50 and called <= set(_lib.ENTRIES), called - set(_lib.ENTRIES)


@pytest.mark.parametrize("basename", BASENAMES)
def test_every_entry_is_bound_as_declared(lib, basename):
    for name in NAMES[basename]:
        fn = getattr(lib, name)
        res, args = _lib.ENTRIES[name]
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.cfm_abi_version() == _lib.ABI_VERSION == 4


@pytest.mark.parametrize("basename", BASENAMES)
def test_a_library_without_a_headers_entries_asks_for_a_rebuild(monkeypatch, basename):
    """load() on a stand-in library of the right revision that answers every name except this header's: the message names the
    first missing entry, its header and the remedy.  (The revision check comes first, so the stand-in keeps cfm_abi_version.)"""
    missing = set(NAMES[basename]) - {"cfm_abi_version"}

    class Fn:
        restype = argtypes = None

        def __call__(self, *a):
            return _lib.ABI_VERSION

    class Lib:
        def __getattr__(self, name):
            if name in missing:
                raise AttributeError(name)
            fn = Fn()
            object.__setattr__(self, name, fn)
            return fn

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda *a, **kw: Lib())
    first = re.escape(f"lacks {NAMES[basename][0]} (include/{basename}): rebuild")
    with pytest.raises(_lib.ConformerHipError, match=first):
        _lib.load()
    assert _lib._lib is None


def test_a_library_of_another_revision_is_refused_first(monkeypatch):
    class Lib:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda *a, **kw: Lib())
    with pytest.raises(_lib.ConformerHipError, match="implements C-ABI revision 0, this binding needs 4"):
        _lib.load()
    assert _lib._lib is None


def test_a_missing_or_duplicated_header_is_refused(tmp_path):
    absent = str(tmp_path / "conformer_hip_absent.h")
    with pytest.raises(_lib.ConformerHipError, match=re.escape(f"{absent} is missing: the ctypes binding is derived from it")):
        _lib.read_header(absent)
    again = tmp_path / "conformer_hip_again.h"
    again.write_text("int cfm_brand_new(int x);\nint cfm_version(void);\n#define CFM_AGAIN 3\n")
    with pytest.raises(_lib.ConformerHipError, match=re.escape(f"{again} declares again: ['cfm_version']")):
        _lib.read_header(str(again), _lib.ENTRIES)
    header = _lib.read_header(str(again))                                 # nothing read before it: it stands
    assert header.path == str(again) and list(header.signatures) == ["cfm_brand_new", "cfm_version"]
    assert header.params["cfm_brand_new"] == ["x"] and header.constants == {"CFM_AGAIN": 3}


def test_build_depends_on_every_header():
    from conformer_amd import build
    deps = build.dependencies()
    csrc = os.path.join(ROOT, "conformer_amd", "csrc")
    inner = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    assert inner and len(deps) == len(set(deps))
    assert set(deps) == {header.path for header in _lib.HEADERS.values()} | set(inner)
    assert all(build._newest_dep() >= os.path.getmtime(header.path) for header in _lib.HEADERS.values())
    assert build._newest_dep() == max(os.path.getmtime(d) for d in deps)


def test_build_sizes_its_compile_pool(monkeypatch):
    from conformer_amd import build
    monkeypatch.setenv("MAX_JOBS", "16")
    assert build._jobs(39) == 16 and build._jobs(3) == 3
    monkeypatch.setenv("MAX_JOBS", "2")
    assert build._jobs(39) == 2
    monkeypatch.delenv("MAX_JOBS")
    monkeypatch.setattr(os, "cpu_count", lambda: 384)
    assert build._jobs(39) == 16 and build._jobs(5) == 5
    monkeypatch.setattr(os, "cpu_count", lambda: None)
    assert build._jobs(39) == 4


@pytest.mark.parametrize("basename", ["conformer_hip.h", "conformer_hip_times.h"])
def test_the_build_hook_resolves_every_entry_of_the_table(lib, monkeypatch, basename):
    """An entry added to a header's record and nothing else: __graft_entry__.build() fails, whether the library is already
    loaded (its own loop over ENTRIES) or not (load())."""
    import __graft_entry__ as entry
    from conformer_amd import build
    built = []
    monkeypatch.setattr(build, "build_library", lambda force=False, verbose=True: built.append(force))
    entry.build()                                                          # the table as it is resolves
    assert built == [False]
    fake = (ctypes.c_int, [])
    monkeypatch.setitem(_lib.HEADERS[basename].signatures, "cfm_not_built_yet", fake)
    monkeypatch.setitem(_lib.ENTRIES, "cfm_not_built_yet", fake)
    with pytest.raises(AttributeError, match="cfm_not_built_yet"):
        entry.build()
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.ConformerHipError, match=rf"lacks cfm_not_built_yet \(include/{basename}\): rebuild"):
        entry.build()
    assert _lib._lib is None and built == [False] * 3
