"""ctypes binding of libconformer_hip.so, derived from the one statement of its C ABI: include/conformer_hip.h and the extension
headers listed in EXTENSION_HEADERS.

Every header is parsed once at import (no torch needed) into HEADERS; ENTRIES and PARAMS span all of them, SIGNATURES and
CONSTANTS are the main header's declarations and its `#define CFM_*` lines and `enum cfm_status`.  A type the parser does not
know, or a `cfm_*(` it cannot read, is an error, never a guess.  There is NO fallback: a missing header or library, or a
non-zero status, raises.  Nothing here imports the CPU oracle.

That table is the first generation and is closed.  Families added after it are the second generation (EXTRA_HEADERS: symbols
cfm2_*, defines CFM2_*, one header per family in conformer_amd/csrc/), parsed by the same parser into EXTRA_ENTRIES, EXTRA_PARAMS
and EXTRA_CONSTANTS and bound by `load` after the first, with the same refusal of a library that lacks one.  That table is
closed too (one family, CTC forced alignment without a length limit).

The third generation is OPEN: every conformer_amd/csrc/conformer_hip3_<family>.h (symbols cfm3_*, defines CFM3_*) is discovered
from the directory, in sorted order, parsed into OPEN_ENTRIES, OPEN_PARAMS and OPEN_CONSTANTS and bound by `load` after the
second generation.  A new family is its header in csrc/ and its `extern "C"` definitions in a .hip file there: no list here or
anywhere else names it.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
# (CONFORMER_AMD_LIB: A/B a differently built library from tools/*, development only)
LIB_PATH = os.environ.get("CONFORMER_AMD_LIB") or os.path.join(_HERE, "lib", "libconformer_hip.so")
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
MAIN_HEADER = "conformer_hip.h"             # ABI_VERSION and enum cfm_status come from this one
HEADER_PATH = os.path.join(_INCLUDE, MAIN_HEADER)
# entry families added to the library without touching the main header (no existing signature moves, so the ABI revision
# stays), in the order they were added.  A new family is its header under include/, its .hip file and one line here.
EXTENSION_HEADERS = (
    "conformer_hip_window.h",               # bounded-history attention over ring K/V caches
    "conformer_hip_commit.h",               # the committed-prefix streaming search
    "conformer_hip_times.h",                # token timestamps from the resumable beam search
    "conformer_hip_stream_frontend.h",      # the staging entry of the streaming audio front end
    "conformer_hip_resample.h",             # the resampler in front of the audio front end
    "conformer_hip_endpoint.h",             # endpointing on the blank posterior
    "conformer_hip_error_rate.h",           # error counts (WER / CER / token error rate)
    "conformer_hip_confidence.h",           # token and word confidence (its defines name the methods and aggregations)
)
_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
           "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "cfm_stream_t": ctypes.c_void_p}
# second generation: families added after the first-generation table (the nine headers under include/, their cfm_* entries
# and CFM_* defines) was closed.  Symbols cfm2_*, defines CFM2_*, one header per family beside the kernels in csrc/.
EXTRA_HEADERS = (
    os.path.join(_HERE, "csrc", "conformer_hip2_align_long.h"),     # CTC forced alignment without a length limit
)
EXTRA_PREFIX = "cfm2_"
# third generation, open: whatever conformer_hip3_*.h lies beside the kernels
OPEN_PREFIX = "cfm3_"
OPEN_HEADERS = tuple(sorted(os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))
                            if f.startswith("conformer_hip3_") and f.endswith(".h")))


class ConformerHipError(RuntimeError):
    pass


def parse_header(text: str, prefix: str = "cfm_"):
    """(SIGNATURES, PARAMS, CONSTANTS) of the header `text`: name -> (restype, [argtypes]), name -> [parameter names]
    (`arg<i>` where the header names none), and every `#define CFM_X <integer>` / `CFM_X = <integer>` enum member -> int.
    `prefix`: what the entries' names start with; the defines read start with its upper case ("cfm2_": cfm2_* and CFM2_*)."""
    fn, define = re.escape(prefix), re.escape(prefix.upper())

    def ctype(words, where):            # words: the type without `const`, every `*` glued to the word before it
        if words[-1].endswith("*"):
            return ctypes.c_void_p
        if " ".join(words) not in _CTYPES:
            raise ConformerHipError(f"{HEADER_PATH}: {where}: no ctypes mapping for the type `{' '.join(words)}`")
        return _CTYPES[" ".join(words)]

    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    signatures, params = {}, {}
    for ret, name, plist in re.findall(rf"^[ \t]*((?:const\s+)?\w+[\s*]+?)({fn}\w+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        ret = re.sub(r"\s*\*\s*", "* ", ret).split()
        restype = ctypes.c_char_p if ret == ["const", "char*"] else ctype(ret, name)
        argtypes, names = [], []
        for i, p in enumerate([] if plist.strip() in ("", "void") else plist.split(",")):
            words = [w for w in re.sub(r"\s*\*\s*", "* ", p).split() if w != "const"]
            named = len(words) > 1 and re.fullmatch(r"[A-Za-z_]\w*", words[-1]) is not None
            argtypes.append(ctype(words[:-1] if named else words, f"{name}, parameter {i + 1} `{p.strip()}`"))
            names.append(words[-1] if named else f"arg{i}")
        signatures[name], params[name] = (restype, argtypes), names
    tokens = re.findall(rf"{fn}\w+\s*\(", text)
    if len(tokens) != len(signatures):           # a declaration the pattern above did not read (or read twice)
        missed = sorted({t.rstrip("( \t\n") for t in tokens} - set(signatures)) or "a duplicate"
        raise ConformerHipError(f"{HEADER_PATH}: {len(tokens)} `{prefix}*(` tokens but {len(signatures)} declarations read: "
                                f"{missed}")
    constants = re.findall(rf"^[ \t]*#[ \t]*define[ \t]+({define}\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)
    constants += re.findall(rf"^[ \t]*({define}\w+)[ \t]*=[ \t]*(-?\d+)[ \t]*,?[ \t]*$", text, flags=re.M)
    return signatures, params, {k: int(v) for k, v in constants}


class Header(NamedTuple):
    """one header of include/: its path and what `parse_header` read from it"""
    path: str
    signatures: dict
    params: dict
    constants: dict


def read_header(path: str, earlier=(), prefix: str = "cfm_") -> Header:
    """Parse the header at `path`; a name it shares with `earlier` (the entries of the headers read before it) is an error."""
    if not os.path.exists(path):
        raise ConformerHipError(f"{path} is missing: the ctypes binding is derived from it")
    with open(path) as f:
        header = Header(path, *parse_header(f.read(), prefix))
    if set(header.signatures) & set(earlier):
        raise ConformerHipError(f"{path} declares again: {sorted(set(header.signatures) & set(earlier))}")
    return header


HEADERS: dict = {}        # basename -> Header, the main header first; an extension header's own defines stay with its record
ENTRIES: dict = {}        # name -> (restype, [argtypes]) over all headers: what `load` binds
PARAMS: dict = {}         # name -> [parameter names] over all headers (`call` names a parameter of any of them)
for _name in (MAIN_HEADER, *EXTENSION_HEADERS):
    HEADERS[_name] = read_header(os.path.join(_INCLUDE, _name), ENTRIES)
    ENTRIES.update(HEADERS[_name].signatures)
    PARAMS.update(HEADERS[_name].params)
SIGNATURES = HEADERS[MAIN_HEADER].signatures      # the main header's entries
CONSTANTS = HEADERS[MAIN_HEADER].constants        # ... and its defines and status codes
ABI_VERSION = CONSTANTS["CFM_ABI_VERSION"]        # checked in load()

EXTRA: dict = {}          # path -> Header of the second-generation headers, in the order of EXTRA_HEADERS
EXTRA_ENTRIES: dict = {}  # name -> (restype, [argtypes]): bound by `load` after ENTRIES
EXTRA_PARAMS: dict = {}   # name -> [parameter names]
EXTRA_CONSTANTS: dict = {}  # basename -> the header's own CFM2_* defines
for _path in EXTRA_HEADERS:
    EXTRA[_path] = read_header(_path, EXTRA_ENTRIES, EXTRA_PREFIX)
    EXTRA_ENTRIES.update(EXTRA[_path].signatures)
    EXTRA_PARAMS.update(EXTRA[_path].params)
    EXTRA_CONSTANTS[os.path.basename(_path)] = EXTRA[_path].constants

OPEN: dict = {}           # path -> Header of the third-generation headers, in the order of OPEN_HEADERS
OPEN_ENTRIES: dict = {}   # name -> (restype, [argtypes]): bound by `load` after EXTRA_ENTRIES
OPEN_PARAMS: dict = {}    # name -> [parameter names]
OPEN_CONSTANTS: dict = {}  # basename -> the header's own CFM3_* defines
for _path in OPEN_HEADERS:
    OPEN[_path] = read_header(_path, OPEN_ENTRIES, OPEN_PREFIX)
    OPEN_ENTRIES.update(OPEN[_path].signatures)
    OPEN_PARAMS.update(OPEN[_path].params)
    OPEN_CONSTANTS[os.path.basename(_path)] = OPEN[_path].constants


def header_of(name: str) -> str:
    """basename of the header that declares the entry `name`"""
    return next(basename for basename, header in HEADERS.items() if name in header.signatures)


_lib = None


def load() -> ctypes.CDLL:
    """Load the library once.  `import torch` first so the HIP runtime torch ships is the one bound."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ConformerHipError(
            f"{LIB_PATH} is missing: build it with `python -m conformer_amd.build` "
            "(there is no CPU/eager fallback for the Conformer hot path)")
    import torch  # noqa: F401  (loads libamdhip64 from torch/lib before our DT_NEEDED is resolved)
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    # a library built against another revision of include/conformer_hip.h would take shifted arguments silently (ctypes checks
    # nothing): refuse it before the first call (matters most for the CONFORMER_AMD_LIB override)
    try:
        lib.cfm_abi_version.restype = ctypes.c_int
        got = int(lib.cfm_abi_version())
    except AttributeError:
        got = 0
    if got != ABI_VERSION:
        raise ConformerHipError(f"{LIB_PATH} implements C-ABI revision {got}, this binding needs {ABI_VERSION}: rebuild it with "
                                "`python -m conformer_amd.build`")
    for basename, header in HEADERS.items():
        for name, (res, args) in header.signatures.items():
            # same ABI revision, newer entry: a library built before an extension header existed passes the check above
            fn = getattr(lib, name, None)
            if fn is None:
                raise ConformerHipError(f"{LIB_PATH} lacks {name} (include/{basename}): rebuild it with "
                                        "`python -m conformer_amd.build`")
            fn.restype = res
            fn.argtypes = args
    for path, header in (*EXTRA.items(), *OPEN.items()):      # the second generation after the first, then the third
        for name, (res, args) in header.signatures.items():
            fn = getattr(lib, name, None)
            if fn is None:
                raise ConformerHipError(f"{LIB_PATH} lacks {name} (csrc/{os.path.basename(path)}): rebuild it with "
                                        "`python -m conformer_amd.build`")
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


class CastItem(ctypes.Structure):
    """cfm_cast_item of include/conformer_hip.h"""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("rows", ctypes.c_int64), ("cols", ctypes.c_int64),
                ("transpose", ctypes.c_int)]


CALLS = [0]          # C-ABI calls checked so far (bench.py reports the count of one forward: one call = one kernel launch there)


def check(status: int, what: str) -> None:
    """Count and check a status that was read from `load()` directly (`call` does both for the package's own calls)."""
    CALLS[0] += 1
    if status != CONSTANTS["CFM_OK"]:
        msg = load().cfm_strerror(status).decode()
        raise ConformerHipError(f"{what} failed: {msg} (status {status})")


def call(name: str, *args) -> None:
    """Call the status-returning entry point `name` and raise unless it returns CFM_OK.  The entry is looked up on the CDLL at
    every call (an attribute swapped onto it is what runs); positional arguments only, converted by the header's argtypes."""
    CALLS[0] += 1
    lib = _lib or load()
    try:
        status = getattr(lib, name)(*args)
    except ctypes.ArgumentError as e:
        i = int(re.search(r"argument (\d+)", str(e)).group(1))
        names = PARAMS.get(name) or EXTRA_PARAMS.get(name) or OPEN_PARAMS[name]
        raise ConformerHipError(f"{name}: argument {i} (`{names[i - 1]}`) has the wrong Python type: {e}") from None
    if status:
        raise ConformerHipError(f"{name} failed: {lib.cfm_strerror(status).decode()} (status {status})")
