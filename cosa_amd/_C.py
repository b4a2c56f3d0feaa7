"""ctypes binding of libcosa_hip.so -- the only way the Python host code reaches the HIP kernels.

include/cosa_hip.h is the ONE declaration of the C ABI: every entry point's signature and every integer COSA_* constant the Python side uses
are parsed from its text (parse_header), nothing is repeated here.  A new entry point is a prototype in the header and its definition in a
.hip file.  Loading FAILS LOUDLY when the shared library or the header is missing: there is no CPU or eager-PyTorch fallback anywhere in
the product path.
"""
import ctypes
import functools
import os
import re
import types

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libcosa_hip.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "cosa_hip.h")
_lib = None

c_void_p, c_int, c_float, c_size_t = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
_SCALARS = {"int": c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "long long": ctypes.c_longlong, "size_t": c_size_t,
            "float": c_float, "double": ctypes.c_double}


class CosaError(RuntimeError):
    pass


def _ctype(fn, ctype, ret=False):
    """the ctypes type of the C type `ctype` of function `fn`: scalars by value, every pointer a c_void_p (the header's type does not say
    whether an address is host or device memory), a `const char *` return a c_char_p; anything else is an error, never a guess"""
    t = " ".join(w for w in ctype.replace("*", " * ").split() if w != "const")
    if ret and t in ("void", "char *"):
        return None if t == "void" else ctypes.c_char_p
    if re.fullmatch(r"[\w ]+( \*)+", t):
        return c_void_p
    if t not in _SCALARS:
        raise CosaError(f"cosa_hip.h: {fn}: unknown type '{ctype}'")
    return _SCALARS[t]


def parse_header(text):
    """-> ({name: (restype, argtypes)}, {COSA_X: int}) from the text of a C header in the style of include/cosa_hip.h"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(COSA_\w+)[ \t]+(\d+)u?[ \t]*$", text, flags=re.M)}
    text = re.sub(r'^[ \t]*#[^\n]*|extern\s+"C"\s*\{|typedef\s+struct\b[^{};]*\{[^{}]*\}[^;]*;', " ", text, flags=re.M)
    sigs = {}
    for stmt in (" ".join(s.split()) for s in text.split(";")):
        if stmt in ("", "}"):                                       # (the closing brace of extern "C")
            continue
        m = re.fullmatch(r"(.+?)\b(\w+) ?\((.*)\)", stmt)
        if not m:
            raise CosaError(f"cosa_hip.h: cannot parse '{stmt}'")
        ret, fn, args = m.groups()
        params = [] if args.strip() == "void" else [re.fullmatch(r"(.+?)\b\w+", a.strip()) for a in args.split(",")]
        if not all(params):
            raise CosaError(f"cosa_hip.h: {fn}: cannot parse the parameters '{args}'")
        sigs[fn] = (_ctype(fn, ret, ret=True), [_ctype(fn, p[1]) for p in params])
    return sigs, types.MappingProxyType(consts)


@functools.lru_cache(maxsize=None)
def _header():
    if not os.path.exists(HEADER_PATH):
        raise CosaError(f"{HEADER_PATH} is missing: the binding takes every signature and constant from it")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


def declared_symbols():
    return list(_header()[0])


def constant(name):
    """the integer `#define COSA_...` of include/cosa_hip.h"""
    return _header()[1][name]


# the fp16-operand builds of the GEMM / attention translation units export the same signatures under other names: THE table of the twins whose
# name is not `name + "_f16"`, plus the attention backward's pair, which is regular but listed so that every 16-bit entry point a test picks
# by dtype is named in one place (fn16 resolves through it)
_F16_TWIN = {"cosa_gemm_bf16": "cosa_gemm_f16", "cosa_gemm_wgrad_bf16": "cosa_gemm_wgrad_f16",
             # fp16x3 (round 6): the three-term GEMM / attention with fp16 halves
             "cosa_gemm_bf16x3": "cosa_gemm_f16x3", "cosa_attn_fwd_bf16x3": "cosa_attn_fwd_f16x3",
             # the student's attention backward: the fp16 build of the same three kernels
             "cosa_attn_bwd": "cosa_attn_bwd_f16", "cosa_attn_bwd_workspace_bytes": "cosa_attn_bwd_workspace_bytes_f16"}


def fn16(name, dtype):
    """the entry point `name` for 16-bit operands (or split halves: bf16x3 -> fp16x3) of torch dtype `dtype`: bf16 -> name, fp16 -> its twin"""
    if dtype == torch.bfloat16:
        return getattr(lib(), name)
    if dtype == torch.float16:
        return getattr(lib(), _F16_TWIN.get(name, name + "_f16"))
    raise CosaError(f"{name}: operands must be bfloat16 or float16, got {dtype}")


def load(path, strict=True):
    """Open the library at `path` and give every entry point of the header its restype / argtypes.  A name the library lacks is an error, or
    with strict=False left unset (an older build in an A/B run)."""
    L = ctypes.CDLL(path)
    for name, (res, args) in _header()[0].items():
        try:
            fn = getattr(L, name)
        except AttributeError as e:
            if not strict:
                continue
            raise CosaError(f"{os.path.basename(path)} does not export {name} (stale build?)") from e
        fn.restype = res
        fn.argtypes = args
    return L


def lib():
    """Load libcosa_hip.so (once).  Raises CosaError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CosaError(
                f"{LIB_PATH} is missing: build the HIP extension first (python -m cosa_amd.build). "
                "cosa_amd has no CPU fallback.")
        _lib = load(LIB_PATH)
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().cosa_last_error().decode("utf-8", "replace")
        raise CosaError(f"{what} failed (code {rc}): {msg}")


def stream_ptr():
    """Raw hipStream_t of torch's current stream (so kernels order with torch ops)."""
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise CosaError("cosa_amd operators need device (HIP) tensors; there is no CPU path")


_ws_cache = {}
_ws_scope = ""


class workspace_scope:
    """`with workspace_scope("name"):` -- workspace() calls inside take slots of their own ("name/<tag>").  For a second network that runs
    between the steps of a trainer whose captured graph holds the addresses of the default slots (the --teacher_check pass): a larger request
    of its own can then never replace, and so free, a buffer that graph replays into.  Outside a scope the keys are what they always were."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        global _ws_scope
        self.prev, _ws_scope = _ws_scope, self.name + "/"
        return self

    def __exit__(self, *exc):
        global _ws_scope
        _ws_scope = self.prev
        return False


def workspace(nbytes, device, tag="default"):
    """Grow-only per-(device,tag) byte workspace (never freed inside the step: graph-safe)."""
    key = (str(device), _ws_scope + tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


# ---- optional per-kernel HIP-event timing (bench.py's roofline leg) ------------------------------------
_prof = None


def profile_start():
    """Record a HIP event pair around every profiled() region on torch's current stream (= the launch stream)."""
    global _prof
    _prof = {}


def profile_stop():
    """-> {name: (n_launches, total_ms)}; synchronises."""
    global _prof
    p, _prof = _prof, None
    torch.cuda.synchronize()
    out = {}
    for k, v in (p or {}).items():
        n, ms = 0, 0.0
        for a, b in v:
            try:
                ms += a.elapsed_time(b)
                n += 1
            except RuntimeError:                 # an event pair that cannot be timed must not take the measurement down
                pass
        out[k] = (n, ms)
    return out


class profiled:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.on = _prof is not None and not torch.cuda.is_current_stream_capturing()    # events inside a graph capture cannot be timed
        if self.on:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        if self.on and _prof is not None:
            self.b.record()
            _prof.setdefault(self.name, []).append((self.a, self.b))
        return False


def int_array(values):
    arr = (c_int * len(values))(*[int(v) for v in values])
    return arr
