"""Argument rules of the projection GEMM entry points (csrc/gemm_kernels.hip): every refusal happens on the host, before the first HIP call,
with COSA_EINVAL and the message of the broken rule.  No GPU.

NO VALID CALL MAY EVER BE ADDED TO THIS FILE.  The non-null pointers are addresses inside a small host buffer: a call that passed the
checks would launch a kernel on them.  `refused` therefore restates the rules (`broken_rules`) and does not make a call that breaks none."""
import ctypes

import pytest

EINVAL = 1
M, N, K = 256, 256, 256                     # satisfies every entry's tile rule (c4: K >= 256, K % 256 == 0)
POINTERS = {"gemm": ("X", "W", "bias", "Y"), "x3": ("X", "W", "bias", "Y"), "c8": ("X", "W", "bias", "Y"),
            "c4": ("X", "Xscales", "W", "Wscales", "bias", "Y"), "dual": ("X", "W", "bias", "H", "A")}
# entry point -> (kind, name in its messages: the fp16 builds report under the bf16 names, N multiple, K multiple)
ENTRIES = {"cosa_gemm_bf16": ("gemm", "cosa_gemm_bf16", 128, 64), "cosa_gemm_f16": ("gemm", "cosa_gemm_bf16", 128, 64),
           "cosa_gemm_bf16x3": ("x3", "cosa_gemm_bf16x3", 128, 64), "cosa_gemm_f16x3": ("x3", "cosa_gemm_bf16x3", 128, 64),
           "cosa_gemm_f16c8": ("c8", "cosa_gemm_f16c8", 256, 128), "cosa_gemm_f16c4": ("c4", "cosa_gemm_f16c4", 256, 256),
           "cosa_gemm_bf16_dual_gelu": ("dual", "cosa_gemm_bf16_dual_gelu", 128, 64)}
# the words of the N / K rule's message per kind, as printf renders them
SHAPE_WORDS = {"gemm": "N must be a multiple of 128 and K of 64", "x3": "N % 128 and K % 64 must be 0", "dual": "N % 128 and K % 64 must be 0",
               "c8": "N % 256 == 0 and K % 128 == 0 required", "c4": "N % 256 == 0 and K % 256 == 0 required"}


@pytest.fixture(scope="module")
def L():
    from cosa_amd import _C, build
    build.build_all()
    return _C.lib()


def good_ldy(kind, epilogue):
    if kind == "x3":
        return N if epilogue == 2 else 2 * N
    return N if epilogue != 1 else 2 * N + 64


def broken_rules(kind, tile_n, step_k, a):
    """the rules of the entry points, restated: the names of those that the arguments `a` break"""
    bad = []
    if any(not a[p] for p in POINTERS[kind]):
        bad.append("null")
    if kind == "dual" and a["H"] == a["A"]:
        bad.append("alias")
    if min(a["M"], a["N"], a["K"]) <= 0 or a["N"] % tile_n or a["K"] % step_k or (kind == "c4" and a["K"] < 256):
        bad.append("shape")
    if kind == "dual":
        return bad
    e = a["epilogue"]
    if not 0 <= e <= 2:
        bad.append("epilogue")
    if e == 2 and not a["residual"]:
        bad.append("residual")
    if kind == "c4" and e == 1 and not a["Yscales"]:
        bad.append("yscales")
    if kind == "x3" and not (a["ldy"] == a["N"] if e == 2 else (a["ldy"] >= 2 * a["N"] and a["ldy"] % 8 == 0)):
        bad.append("ldy")
    if kind in ("c8", "c4") and not (a["ldy"] == a["N"] if e == 2 else a["ldy"] == 2 * a["N"] + 64 if e == 1 else (a["ldy"] >= a["N"] and a["ldy"] % 8 == 0)):
        bad.append("ldy")
    return bad


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_broken_rule_is_refused_on_the_host(L, entry):
    kind, who, tile_n, step_k = ENTRIES[entry]
    host = ctypes.create_string_buffer(1024)
    at = lambda i: ctypes.addressof(host) + 64 * i
    base = dict(X=at(0), Xscales=at(1), W=at(2), Wscales=at(3), bias=at(4), residual=at(5), Y=at(6), Yscales=at(7), H=at(8), A=at(9),
                M=M, N=N, K=K, epilogue=0)
    fn = getattr(L, entry)

    def refused(words, **change):
        a = dict(base, **change)
        a.setdefault("ldy", good_ldy(kind, a["epilogue"]))
        assert broken_rules(kind, tile_n, step_k, a), (entry, change)          # never a valid call: see the module docstring
        if kind == "gemm":
            rc = fn(a["X"], a["W"], a["bias"], a["residual"], a["Y"], a["M"], a["N"], a["K"], a["epilogue"], None)
        elif kind in ("x3", "c8"):
            rc = fn(a["X"], a["W"], a["bias"], a["residual"], a["Y"], a["M"], a["N"], a["K"], a["epilogue"], a["ldy"], None)
        elif kind == "c4":
            rc = fn(a["X"], a["Xscales"], a["W"], a["Wscales"], a["bias"], a["residual"], a["Y"], a["Yscales"], a["M"], a["N"], a["K"],
                    a["epilogue"], a["ldy"], None)
        else:
            rc = fn(a["X"], a["W"], a["bias"], a["H"], a["A"], a["M"], a["N"], a["K"], None)
        assert rc != 0, (entry, change)
        msg = L.cosa_last_error().decode()
        assert rc == EINVAL and msg.startswith(who + ": ") and all(w in msg for w in words), (entry, change, rc, msg)

    for p in POINTERS[kind]:
        refused(["null pointer"], **{p: None})
    refused([SHAPE_WORDS[kind], f"N={N - 64}", f"K={K}"], N=N - 64)
    refused([SHAPE_WORDS[kind], f"N={N}", f"K={K - 32}"], K=K - 32)
    if kind == "dual":
        refused(["null pointer", "aliased outputs"], A=base["H"])
        return
    refused(["unknown epilogue"], epilogue=3)
    refused(["unknown epilogue"], epilogue=-1)
    refused(["residual epilogue needs the residual pointer"], epilogue=2, residual=None)
    if kind == "x3":
        for e, ldy in ((0, 2 * N - 8), (1, 2 * N + 4), (2, 2 * N)):
            refused(["ldy must be N (fp32 out) or >= 2N (split out)"], epilogue=e, ldy=ldy)
    if kind in ("c8", "c4"):
        rows = "c8 rows out" if kind == "c8" else "c4 rows out"
        for e, ldy in ((0, N - 8), (0, N + 4), (1, 2 * N), (2, 2 * N + 64)):
            refused([f"ldy must be N (fp32 out), 2N + 64 ({rows}) or >= N (fp16 out)"], epilogue=e, ldy=ldy)
    if kind == "c4":
        refused(["GELU epilogue", "needs their scale tensor"], epilogue=1, Yscales=None)
