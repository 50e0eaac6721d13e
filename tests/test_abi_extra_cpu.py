"""The second-generation entry table (`_lib.EXTRA_*`: symbols cfm2_*, defines CFM2_*, headers beside the kernels in csrc/): what
the sources define, what the headers declare and what the binding binds are one set, disjoint from the first generation, which
stays exactly as tests/test_abi.py and tests/test_abi_binding_cpu.py pin it."""
import ctypes
import os
import re

import pytest

from conformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conformer_amd", "csrc")
NAMES = {
    "conformer_hip2_align_long.h": ["cfm2_ctc_align_long_workspace_bytes", "cfm2_ctc_align_long_launches",
                                    "cfm2_ctc_align_long_f32", "cfm2_ctc_align_long_chain_f32"],
}


@pytest.fixture(scope="module")
def lib():
    from conformer_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


def defined():
    """name -> number of parameters of every `extern "C"` cfm2_* definition in csrc/*.hip (a source scan, no library needed)"""
    out = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hip"):
            out += re.findall(r'extern\s+"C"[^;{()]*?\b(cfm2_\w+)\s*\(([^()]*)\)\s*\{', open(os.path.join(CSRC, f)).read())
    assert len(out) == len({name for name, _ in out})
    return {name: 0 if args.strip() in ("", "void") else len(args.split(",")) for name, args in out}


def test_the_table_names_every_second_generation_header():
    assert [os.path.basename(p) for p in _lib.EXTRA_HEADERS] == list(NAMES) == list(_lib.EXTRA_CONSTANTS)
    assert all(os.path.dirname(p) == CSRC for p in _lib.EXTRA_HEADERS)
    second = sorted(f for f in os.listdir(CSRC) if f.startswith("conformer_hip2_") and f.endswith(".h"))
    assert second == sorted(NAMES)                                        # a header nobody registered fails here
    assert list(_lib.EXTRA_ENTRIES) == [name for listed in NAMES.values() for name in listed]
    assert set(_lib.EXTRA_PARAMS) == set(_lib.EXTRA_ENTRIES)
    from conformer_amd import build
    assert set(_lib.EXTRA_HEADERS) <= set(build.dependencies())


def test_declared_equals_defined_with_the_same_arity():
    d = defined()
    assert set(d) == set(_lib.EXTRA_ENTRIES), set(d) ^ set(_lib.EXTRA_ENTRIES)
    for name, n in d.items():
        assert len(_lib.EXTRA_ENTRIES[name][1]) == n == len(_lib.EXTRA_PARAMS[name]), name


def test_no_overlap_with_the_first_generation():
    assert not set(_lib.EXTRA_ENTRIES) & set(_lib.ENTRIES)
    assert all(name.startswith("cfm2_") for name in _lib.EXTRA_ENTRIES)
    assert not any(name.startswith("cfm2_") for name in _lib.ENTRIES)
    for constants in _lib.EXTRA_CONSTANTS.values():
        assert all(k.startswith("CFM2_") for k in constants) and not set(constants) & set(_lib.CONSTANTS)
    assert _lib.EXTRA_CONSTANTS["conformer_hip2_align_long.h"] == {"CFM2_CTC_ALIGN_LONG_MAX_FRAMES": 1048576,
                                                                   "CFM2_CTC_ALIGN_LONG_MAX_TARGET": 262143}


def test_the_first_generation_is_unchanged_in_size():
    assert (len(_lib.HEADERS), len(_lib.ENTRIES), len(_lib.PARAMS)) == (9, 162, 162)
    assert len(_lib.SIGNATURES) == 144 and _lib.ABI_VERSION == 4
    assert not any(os.path.basename(p) in _lib.HEADERS for p in _lib.EXTRA_HEADERS)


def test_parse_header_with_a_prefix():
    text = """/* cfm2_in_a_comment(int x); */
    #define CFM2_LIMIT 12
    #define CFM_OLD 3
    int cfm_old(int x);
    size_t cfm2_bytes(int B, const float* x);
    """
    sig, params, constants = _lib.parse_header(text, "cfm2_")
    assert sig == {"cfm2_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_void_p])}
    assert params == {"cfm2_bytes": ["B", "x"]} and constants == {"CFM2_LIMIT": 12}
    sig, params, constants = _lib.parse_header(text)                      # one argument: the first generation, as ever
    assert list(sig) == ["cfm_old"] and constants == {"CFM_OLD": 3}
    with pytest.raises(_lib.ConformerHipError, match="no ctypes mapping"):
        _lib.parse_header("int cfm2_x(struct y z);", "cfm2_")
    with pytest.raises(_lib.ConformerHipError, match=r"`cfm2_\*\(` tokens"):
        _lib.parse_header("int cfm2_x(int (*f)(int));", "cfm2_")


def test_every_entry_is_bound_as_declared(lib):
    for name, (res, args) in _lib.EXTRA_ENTRIES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    res, args = _lib.EXTRA_ENTRIES["cfm2_ctc_align_long_f32"]
    assert res is ctypes.c_int and len(args) == 21 and args[9:13] == [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    assert _lib.EXTRA_PARAMS["cfm2_ctc_align_long_f32"][9:13] == ["tile_pairs", "chunk_frames", "workspace", "workspace_bytes"]
    first = _lib.PARAMS["cfm_ctc_align_f32"]                              # the arguments of cfm_ctc_align_f32 plus the two
    assert _lib.EXTRA_PARAMS["cfm2_ctc_align_long_f32"] == first[:9] + ["tile_pairs", "chunk_frames"] + first[9:]


@pytest.mark.parametrize("missing", [name for listed in NAMES.values() for name in listed])
def test_a_library_without_an_entry_asks_for_a_rebuild(monkeypatch, missing):
    """load() on a stand-in library that answers every name but one of the second generation: the first generation binds, then
    the message names the entry, its header and the remedy."""
    asked = []

    class Fn:
        restype = argtypes = None

        def __call__(self, *a):
            return _lib.ABI_VERSION

    class Lib:
        def __getattr__(self, name):
            asked.append(name)
            if name == missing:
                raise AttributeError(name)
            fn = Fn()
            object.__setattr__(self, name, fn)
            return fn

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda *a, **kw: Lib())
    with pytest.raises(_lib.ConformerHipError, match=re.escape(f"lacks {missing} (csrc/conformer_hip2_align_long.h): rebuild")):
        _lib.load()
    assert _lib._lib is None
    assert set(_lib.ENTRIES) <= set(asked[:asked.index(missing)])         # bound after the first-generation loop


def test_call_names_a_parameter_of_either_table(lib):
    with pytest.raises(_lib.ConformerHipError, match=r"cfm2_ctc_align_long_f32: argument 10 \(`tile_pairs`\)"):
        _lib.call("cfm2_ctc_align_long_f32", *([None] * 4), *([1] * 5), "512", *([0] * 11))
    with pytest.raises(_lib.ConformerHipError, match=r"cfm_ctc_align_f32: argument 5 \(`B`\)"):
        _lib.call("cfm_ctc_align_f32", *([None] * 4), "2", *([0] * 14))


def test_the_build_hook_resolves_every_second_generation_entry(lib, monkeypatch):
    import __graft_entry__ as entry
    from conformer_amd import build
    monkeypatch.setattr(build, "build_library", lambda force=False, verbose=True: None)
    entry.build()
    monkeypatch.setitem(_lib.EXTRA_ENTRIES, "cfm2_not_built_yet", (ctypes.c_int, []))
    with pytest.raises(AttributeError, match="cfm2_not_built_yet"):
        entry.build()
