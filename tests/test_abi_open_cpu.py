"""The third-generation entry table (`_lib.OPEN_*`: symbols cfm3_*, defines CFM3_*, headers conformer_hip3_<family>.h beside the
kernels in csrc/).  It is OPEN: the headers are discovered from the directory, so nothing here lists a family; what the sources
define, what the headers declare and what the binding binds must be one set, disjoint from the two closed generations, which
keep their sizes.  The argument checks of the wildcard alignment entries (conformer_hip3_align_wild.h) return before any HIP
call, so they run here too."""
import ctypes
import math
import os
import re

import pytest

from conformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conformer_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from conformer_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


def defined():
    """name -> number of parameters of every `extern "C"` cfm3_* definition in csrc/*.hip (a source scan, no library needed)"""
    out = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hip"):
            out += re.findall(r'extern\s+"C"[^;{()]*?\b(cfm3_\w+)\s*\(([^()]*)\)\s*\{', open(os.path.join(CSRC, f)).read())
    assert len(out) == len({name for name, _ in out})
    return {name: 0 if args.strip() in ("", "void") else len(args.split(",")) for name, args in out}


def test_the_table_is_discovered_from_the_directory():
    third = sorted(f for f in os.listdir(CSRC) if f.startswith("conformer_hip3_") and f.endswith(".h"))
    assert third and [os.path.basename(p) for p in _lib.OPEN_HEADERS] == third == list(_lib.OPEN_CONSTANTS)
    assert all(os.path.dirname(p) == CSRC for p in _lib.OPEN_HEADERS) and list(_lib.OPEN) == list(_lib.OPEN_HEADERS)
    assert set(_lib.OPEN_PARAMS) == set(_lib.OPEN_ENTRIES)
    assert list(_lib.OPEN_ENTRIES) == [n for p in _lib.OPEN_HEADERS for n in _lib.OPEN[p].signatures]
    from conformer_amd import build
    assert set(_lib.OPEN_HEADERS) <= set(build.dependencies())


def test_declared_equals_defined_with_the_same_arity():
    d = defined()
    assert set(d) == set(_lib.OPEN_ENTRIES), set(d) ^ set(_lib.OPEN_ENTRIES)
    for name, n in d.items():
        assert len(_lib.OPEN_ENTRIES[name][1]) == n == len(_lib.OPEN_PARAMS[name]), name


def test_disjoint_from_both_closed_tables_which_keep_their_sizes():
    assert not set(_lib.OPEN_ENTRIES) & (set(_lib.ENTRIES) | set(_lib.EXTRA_ENTRIES))
    assert all(name.startswith("cfm3_") for name in _lib.OPEN_ENTRIES)
    assert not any(name.startswith("cfm3_") for name in (*_lib.ENTRIES, *_lib.EXTRA_ENTRIES))
    for constants in _lib.OPEN_CONSTANTS.values():
        assert all(k.startswith("CFM3_") for k in constants) and not set(constants) & set(_lib.CONSTANTS)
    assert (len(_lib.HEADERS), len(_lib.ENTRIES), len(_lib.PARAMS)) == (9, 162, 162)
    assert (len(_lib.EXTRA_HEADERS), len(_lib.EXTRA_ENTRIES), len(_lib.EXTRA_PARAMS)) == (1, 4, 4)
    assert not any(os.path.basename(p) in _lib.HEADERS for p in _lib.OPEN_HEADERS)
    assert not set(_lib.OPEN_HEADERS) & set(_lib.EXTRA_HEADERS)


def test_the_wildcard_family():
    assert _lib.OPEN_CONSTANTS["conformer_hip3_align_wild.h"] == {"CFM3_CTC_ALIGN_WILDCARD": -2}
    first, second = _lib.PARAMS["cfm_ctc_align_f32"], _lib.EXTRA_PARAMS["cfm2_ctc_align_long_f32"]
    assert _lib.OPEN_PARAMS["cfm3_ctc_align_wild_f32"] == first[:9] + ["wildcard_penalty"] + first[9:]
    assert _lib.OPEN_PARAMS["cfm3_ctc_align_long_wild_f32"] == second[:9] + ["wildcard_penalty"] + second[9:]
    assert _lib.OPEN_ENTRIES["cfm3_ctc_align_wild_f32"][1][9] is ctypes.c_float
    assert _lib.OPEN_ENTRIES["cfm3_ctc_align_long_wild_f32"][1][9] is ctypes.c_float
    assert _lib.OPEN_PARAMS["cfm3_ctc_align_wild_workspace_bytes"] == ["B", "T", "Lmax"]
    assert _lib.OPEN_PARAMS["cfm3_ctc_align_long_wild_workspace_bytes"] == ["B", "T", "Lmax", "tile_pairs", "chunk_frames"]
    from conformer_amd import align
    assert align.WILDCARD == -2


def test_every_entry_is_bound_as_declared(lib):
    for name, (res, args) in _lib.OPEN_ENTRIES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


@pytest.mark.parametrize("missing", sorted(_lib.OPEN_ENTRIES))
def test_a_library_without_an_entry_asks_for_a_rebuild(monkeypatch, missing):
    """load() on a stand-in library that answers every name but one of the third generation: the two closed generations bind,
    then the message names the entry, its header and the remedy."""
    asked = []
    header = next(os.path.basename(p) for p, h in _lib.OPEN.items() if missing in h.signatures)

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
    with pytest.raises(_lib.ConformerHipError, match=re.escape(f"lacks {missing} (csrc/{header}): rebuild")):
        _lib.load()
    assert _lib._lib is None
    assert set(_lib.ENTRIES) | set(_lib.EXTRA_ENTRIES) <= set(asked[:asked.index(missing)])    # bound after both


def test_call_names_a_parameter_of_the_open_table(lib):
    with pytest.raises(_lib.ConformerHipError, match=r"cfm3_ctc_align_wild_f32: argument 10 \(`wildcard_penalty`\)"):
        _lib.call("cfm3_ctc_align_wild_f32", *([None] * 4), *([1] * 5), "0.5", *([0] * 10))
    with pytest.raises(_lib.ConformerHipError, match=r"cfm3_ctc_align_long_wild_f32: argument 11 \(`tile_pairs`\)"):
        _lib.call("cfm3_ctc_align_long_wild_f32", *([None] * 4), *([1] * 5), 0.5, "512", *([0] * 11))
    with pytest.raises(_lib.ConformerHipError, match=r"cfm2_ctc_align_long_f32: argument 10 \(`tile_pairs`\)"):
        _lib.call("cfm2_ctc_align_long_f32", *([None] * 4), *([1] * 5), "512", *([0] * 11))


def test_the_build_hook_resolves_every_open_entry(lib, monkeypatch):
    import __graft_entry__ as entry
    from conformer_amd import build
    monkeypatch.setattr(build, "build_library", lambda force=False, verbose=True: None)
    entry.build()
    path = _lib.OPEN_HEADERS[0]
    later = _lib.Header(path, {**_lib.OPEN[path].signatures, "cfm3_not_built_yet": (ctypes.c_int, [])}, {}, {})
    monkeypatch.setitem(_lib.OPEN, path, later)
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.ConformerHipError, match=r"lacks cfm3_not_built_yet \(csrc/conformer_hip3_"):
        entry.build()


# ---- conformer_hip3_align_wild.h: sizes and refusals, before any HIP call ----------------------------------------------------

def pad16(n):
    return (n + 15) // 16 * 16


def test_workspace_bytes(lib):
    short, wild = lib.cfm_ctc_align_workspace_bytes, lib.cfm3_ctc_align_wild_workspace_bytes
    for B, T, L in [(1, 1, 1), (3, 7, 3), (32, 249, 60), (3, 2048, 1023), (3, 2048, 1024), (2, 16384, 4096), (5, 301, 64)]:
        assert wild(B, T, L) == pad16(short(B, T, L)) + pad16(4 * B * T), (B, T, L)
    for bad in ((0, 10, 4), (2, 0, 4), (2, 10, 0), (1, 16385, 4), (1, 10, 4097), (-1, 10, 4)):
        assert short(*bad) == 0 and wild(*bad) == 0, bad
    long, long_wild = lib.cfm2_ctc_align_long_workspace_bytes, lib.cfm3_ctc_align_long_wild_workspace_bytes
    for args in [(1, 1, 1, 512, 16), (3, 1400, 1100, 512, 64), (1, 90000, 30000, 0, 0), (2, 17000, 4200, 2048, 512), (65535, 1, 1, 0, 0)]:
        assert long_wild(*args) == long(*args) + pad16(4 * args[0] * args[1]), args
    for bad in ((0, 10, 4, 512, 16), (1, 1048577, 4, 512, 16), (1, 10, 262144, 512, 16), (1, 10, 4, 511, 16), (1, 10, 4, 512, 8),
                (65536, 10, 4, 512, 16)):
        assert long(*bad) == 0 and long_wild(*bad) == 0, bad


def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_double * 8192)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    NULL, SHAPE, UNSUPPORTED, ALIGN = (_lib.CONSTANTS[k] for k in ("CFM_ERR_NULL", "CFM_ERR_BAD_SHAPE", "CFM_ERR_UNSUPPORTED",
                                                                   "CFM_ERR_ALIGN"))
    assert (NULL, SHAPE, UNSUPPORTED) == (-3, -1, -2)
    # the short form: logits, targets, lengths, target_lengths, B, T, V, Lmax, blank, penalty, workspace, bytes, 7 outputs, stream
    n = lib.cfm3_ctc_align_wild_workspace_bytes(2, 8, 3)
    assert 0 < n < 8192 * 8 - 16
    good = [a, a, None, None, 2, 8, 5, 3, 0, 0.5, a, n, a, a, a, a, a, a, a, None]

    def call(entry=lib.cfm3_ctc_align_wild_f32, base=good, **kw):
        args = list(base)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return entry(*args)

    for i in (0, 1, 10, 12, 13, 14, 15, 16, 17, 18):
        assert call(**{f"a{i}": None}) == NULL, i
    assert call(a4=0) == SHAPE and call(a5=0) == SHAPE and call(a6=1) == SHAPE and call(a7=0) == SHAPE
    assert call(a8=-1) == SHAPE and call(a8=5) == SHAPE
    for bad in (-0.5, -1e-30, math.nan, math.inf, -math.inf):
        assert call(a9=bad) == SHAPE, bad                                           # the penalty: finite and >= 0
    assert call(a5=16385) == UNSUPPORTED and call(a7=4097) == UNSUPPORTED
    assert call(a10=a + 8) == ALIGN
    assert call(a11=n - 1) == SHAPE
    assert call(a11=lib.cfm_ctc_align_workspace_bytes(2, 8, 3)) == SHAPE            # the parent's workspace is too small: no w
    # the order: NULL, then shape and penalty, then the limits, then the alignment, then the size
    assert call(a0=None, a9=-1.0) == NULL and call(a9=-1.0, a5=16385) == SHAPE and call(a5=16385, a10=a + 8) == UNSUPPORTED
    assert call(a10=a + 8, a11=n - 1) == ALIGN
    # the long form: tile_pairs, chunk_frames behind the penalty
    m = lib.cfm3_ctc_align_long_wild_workspace_bytes(2, 8, 3, 512, 16)
    assert 0 < m < 8192 * 8 - 16
    good_long = [a, a, None, None, 2, 8, 5, 3, 0, 0.5, 512, 16, a, m, a, a, a, a, a, a, a, None]
    long = dict(entry=lib.cfm3_ctc_align_long_wild_f32, base=good_long)
    for i in (0, 1, 12, 14, 15, 16, 17, 18, 19, 20):
        assert call(**long, **{f"a{i}": None}) == NULL, i
    assert call(**long, a4=0) == SHAPE and call(**long, a6=1) == SHAPE and call(**long, a8=5) == SHAPE
    for bad in (-0.5, math.nan, math.inf):
        assert call(**long, a9=bad) == SHAPE, bad
    assert call(**long, a5=1048577) == UNSUPPORTED and call(**long, a7=262144) == UNSUPPORTED and call(**long, a4=65536) == UNSUPPORTED
    assert call(**long, a10=500) == UNSUPPORTED and call(**long, a11=24) == UNSUPPORTED
    assert call(**long, a12=a + 8) == ALIGN and call(**long, a13=m - 1) == SHAPE
    assert call(**long, a13=lib.cfm2_ctc_align_long_workspace_bytes(2, 8, 3, 512, 16)) == SHAPE
    assert call(**long, a0=None, a9=math.nan) == NULL and call(**long, a9=math.nan, a10=500) == SHAPE
    assert call(**long, a10=500, a12=a + 8) == UNSUPPORTED and call(**long, a12=a + 8, a13=m - 1) == ALIGN
