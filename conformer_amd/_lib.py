"""ctypes binding of libconformer_hip.so, derived from the one statement of its C ABI: include/conformer_hip.h.

The header is parsed once at import (no torch needed): SIGNATURES and PARAMS from its declarations, CONSTANTS from its `#define
CFM_*` lines and `enum cfm_status`.  A type the parser does not know, or a `cfm_*(` it cannot read, is an error, never a guess.
There is NO fallback: a missing header or library, or a non-zero status, raises.  Nothing here imports the CPU oracle.
"""
from __future__ import annotations

import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# (CONFORMER_AMD_LIB: A/B a differently built library from tools/*, development only)
LIB_PATH = os.environ.get("CONFORMER_AMD_LIB") or os.path.join(_HERE, "lib", "libconformer_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "conformer_hip.h")
# entries added to the library without touching the main header (no existing signature moves, so the ABI revision stays)
EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "conformer_hip_window.h")
# the committed-prefix streaming search, added the same way (its own table: EXT_SIGNATURES stays the window header's)
COMMIT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "conformer_hip_commit.h")
_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
           "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "cfm_stream_t": ctypes.c_void_p}
_DECL = re.compile(r"^[ \t]*((?:const\s+)?\w+[\s*]+?)(cfm_\w+)\s*\(([^()]*)\)\s*;", re.M)


class ConformerHipError(RuntimeError):
    pass


def parse_header(text: str):
    """(SIGNATURES, PARAMS, CONSTANTS) of the header `text`: name -> (restype, [argtypes]), name -> [parameter names]
    (`arg<i>` where the header names none), and every `#define CFM_X <integer>` / `CFM_X = <integer>` enum member -> int."""
    def ctype(words, where):            # words: the type without `const`, every `*` glued to the word before it
        if words[-1].endswith("*"):
            return ctypes.c_void_p
        if " ".join(words) not in _CTYPES:
            raise ConformerHipError(f"{HEADER_PATH}: {where}: no ctypes mapping for the type `{' '.join(words)}`")
        return _CTYPES[" ".join(words)]

    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    signatures, params = {}, {}
    for ret, name, plist in _DECL.findall(text):
        ret = re.sub(r"\s*\*\s*", "* ", ret).split()
        restype = ctypes.c_char_p if ret == ["const", "char*"] else ctype(ret, name)
        argtypes, names = [], []
        for i, p in enumerate([] if plist.strip() in ("", "void") else plist.split(",")):
            words = [w for w in re.sub(r"\s*\*\s*", "* ", p).split() if w != "const"]
            named = len(words) > 1 and re.fullmatch(r"[A-Za-z_]\w*", words[-1]) is not None
            argtypes.append(ctype(words[:-1] if named else words, f"{name}, parameter {i + 1} `{p.strip()}`"))
            names.append(words[-1] if named else f"arg{i}")
        signatures[name], params[name] = (restype, argtypes), names
    tokens = re.findall(r"cfm_\w+\s*\(", text)
    if len(tokens) != len(signatures):           # a declaration the pattern above did not read (or read twice)
        missed = sorted({t.rstrip("( \t\n") for t in tokens} - set(signatures)) or "a duplicate"
        raise ConformerHipError(f"{HEADER_PATH}: {len(tokens)} `cfm_*(` tokens but {len(signatures)} declarations read: {missed}")
    constants = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CFM_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)
    constants += re.findall(r"^[ \t]*(CFM_\w+)[ \t]*=[ \t]*(-?\d+)[ \t]*,?[ \t]*$", text, flags=re.M)
    return signatures, params, {k: int(v) for k, v in constants}


if not os.path.exists(HEADER_PATH):
    raise ConformerHipError(f"{HEADER_PATH} is missing: the ctypes binding is derived from it")
with open(HEADER_PATH) as _f:
    SIGNATURES, PARAMS, CONSTANTS = parse_header(_f.read())
ABI_VERSION = CONSTANTS["CFM_ABI_VERSION"]        # checked in load()
if not os.path.exists(EXT_HEADER_PATH):
    raise ConformerHipError(f"{EXT_HEADER_PATH} is missing: the ctypes binding is derived from it")
with open(EXT_HEADER_PATH) as _f:
    EXT_SIGNATURES, _ext_params, _ = parse_header(_f.read())
if set(EXT_SIGNATURES) & set(SIGNATURES):
    raise ConformerHipError(f"{EXT_HEADER_PATH} declares again: {sorted(set(EXT_SIGNATURES) & set(SIGNATURES))}")
PARAMS.update(_ext_params)                        # (`call` names a parameter of either header)
if not os.path.exists(COMMIT_HEADER_PATH):
    raise ConformerHipError(f"{COMMIT_HEADER_PATH} is missing: the ctypes binding is derived from it")
with open(COMMIT_HEADER_PATH) as _f:
    COMMIT_SIGNATURES, _commit_params, _ = parse_header(_f.read())
if set(COMMIT_SIGNATURES) & (set(SIGNATURES) | set(EXT_SIGNATURES)):
    raise ConformerHipError(f"{COMMIT_HEADER_PATH} declares again: "
                            f"{sorted(set(COMMIT_SIGNATURES) & (set(SIGNATURES) | set(EXT_SIGNATURES)))}")
PARAMS.update(_commit_params)
# token timestamps from the resumable beam search, added the same way
TIMES_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "conformer_hip_times.h")
if not os.path.exists(TIMES_HEADER_PATH):
    raise ConformerHipError(f"{TIMES_HEADER_PATH} is missing: the ctypes binding is derived from it")
with open(TIMES_HEADER_PATH) as _f:
    TIMES_SIGNATURES, _times_params, _ = parse_header(_f.read())
_earlier = set(SIGNATURES) | set(EXT_SIGNATURES) | set(COMMIT_SIGNATURES)
if set(TIMES_SIGNATURES) & _earlier:
    raise ConformerHipError(f"{TIMES_HEADER_PATH} declares again: {sorted(set(TIMES_SIGNATURES) & _earlier)}")
PARAMS.update(_times_params)
# the staging entry of the streaming audio front end, added the same way
STREAM_FRONTEND_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "conformer_hip_stream_frontend.h")
if not os.path.exists(STREAM_FRONTEND_HEADER_PATH):
    raise ConformerHipError(f"{STREAM_FRONTEND_HEADER_PATH} is missing: the ctypes binding is derived from it")
with open(STREAM_FRONTEND_HEADER_PATH) as _f:
    STREAM_FRONTEND_SIGNATURES, _stream_frontend_params, _ = parse_header(_f.read())
_earlier |= set(TIMES_SIGNATURES)
if set(STREAM_FRONTEND_SIGNATURES) & _earlier:
    raise ConformerHipError(f"{STREAM_FRONTEND_HEADER_PATH} declares again: {sorted(set(STREAM_FRONTEND_SIGNATURES) & _earlier)}")
PARAMS.update(_stream_frontend_params)
# the resampler in front of the audio front end, added the same way
RESAMPLE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "conformer_hip_resample.h")
if not os.path.exists(RESAMPLE_HEADER_PATH):
    raise ConformerHipError(f"{RESAMPLE_HEADER_PATH} is missing: the ctypes binding is derived from it")
with open(RESAMPLE_HEADER_PATH) as _f:
    RESAMPLE_SIGNATURES, _resample_params, _ = parse_header(_f.read())
_earlier |= set(STREAM_FRONTEND_SIGNATURES)
if set(RESAMPLE_SIGNATURES) & _earlier:
    raise ConformerHipError(f"{RESAMPLE_HEADER_PATH} declares again: {sorted(set(RESAMPLE_SIGNATURES) & _earlier)}")
PARAMS.update(_resample_params)
# endpointing on the blank posterior, added the same way
ENDPOINT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "conformer_hip_endpoint.h")
if not os.path.exists(ENDPOINT_HEADER_PATH):
    raise ConformerHipError(f"{ENDPOINT_HEADER_PATH} is missing: the ctypes binding is derived from it")
with open(ENDPOINT_HEADER_PATH) as _f:
    ENDPOINT_SIGNATURES, _endpoint_params, _ = parse_header(_f.read())
_earlier |= set(RESAMPLE_SIGNATURES)
if set(ENDPOINT_SIGNATURES) & _earlier:
    raise ConformerHipError(f"{ENDPOINT_HEADER_PATH} declares again: {sorted(set(ENDPOINT_SIGNATURES) & _earlier)}")
PARAMS.update(_endpoint_params)
# error counts (WER / CER / token error rate) on the device, added the same way
ERROR_RATE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "conformer_hip_error_rate.h")
if not os.path.exists(ERROR_RATE_HEADER_PATH):
    raise ConformerHipError(f"{ERROR_RATE_HEADER_PATH} is missing: the ctypes binding is derived from it")
with open(ERROR_RATE_HEADER_PATH) as _f:
    ERROR_RATE_SIGNATURES, _error_rate_params, _ = parse_header(_f.read())
_earlier |= set(ENDPOINT_SIGNATURES)
if set(ERROR_RATE_SIGNATURES) & _earlier:
    raise ConformerHipError(f"{ERROR_RATE_HEADER_PATH} declares again: {sorted(set(ERROR_RATE_SIGNATURES) & _earlier)}")
PARAMS.update(_error_rate_params)
# token and word confidence from the frame posteriors, added the same way (its defines name the methods and aggregations)
CONFIDENCE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "conformer_hip_confidence.h")
if not os.path.exists(CONFIDENCE_HEADER_PATH):
    raise ConformerHipError(f"{CONFIDENCE_HEADER_PATH} is missing: the ctypes binding is derived from it")
with open(CONFIDENCE_HEADER_PATH) as _f:
    CONFIDENCE_SIGNATURES, _confidence_params, CONFIDENCE_CONSTANTS = parse_header(_f.read())
_earlier |= set(ERROR_RATE_SIGNATURES)
if set(CONFIDENCE_SIGNATURES) & _earlier:
    raise ConformerHipError(f"{CONFIDENCE_HEADER_PATH} declares again: {sorted(set(CONFIDENCE_SIGNATURES) & _earlier)}")
PARAMS.update(_confidence_params)

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
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for header, table in ((EXT_HEADER_PATH, EXT_SIGNATURES), (COMMIT_HEADER_PATH, COMMIT_SIGNATURES),
                          (TIMES_HEADER_PATH, TIMES_SIGNATURES), (STREAM_FRONTEND_HEADER_PATH, STREAM_FRONTEND_SIGNATURES),
                          (RESAMPLE_HEADER_PATH, RESAMPLE_SIGNATURES), (ENDPOINT_HEADER_PATH, ENDPOINT_SIGNATURES),
                          (ERROR_RATE_HEADER_PATH, ERROR_RATE_SIGNATURES), (CONFIDENCE_HEADER_PATH, CONFIDENCE_SIGNATURES)):
        for name, (res, args) in table.items():
            # same ABI revision, newer entry: a library built before the extension header existed passes the check above
            fn = getattr(lib, name, None)
            if fn is None:
                raise ConformerHipError(f"{LIB_PATH} lacks {name} (include/{os.path.basename(header)}): rebuild it with "
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
        raise ConformerHipError(f"{name}: argument {i} (`{PARAMS[name][i - 1]}`) has the wrong Python type: {e}") from None
    if status:
        raise ConformerHipError(f"{name} failed: {lib.cfm_strerror(status).decode()} (status {status})")
