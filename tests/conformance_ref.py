"""numpy restatement of the pre-registered CAM criterion, rules (a) and (b), as tests/test_precision_gpu.py:675-701 applies it per plane --
the CPU partner of cosa_conformance_planes (csrc/conformance_kernels.hip; DESIGN.md sections 3 and 20).  TEST INFRASTRUCTURE ONLY.

Per active plane of one CAM set, from camA (the mode under test, fp32), cam32 (the fp32 pass), cam64 (float64) and the float64 pass's
peak / rawmax:
    d = max |A - c32|     lit = d / max(max |c32|, 1e-6)     cond = rawmax / peak     own = d peak / max(rawmax, 1e-30)
    e_ref = max |c32 - c64|     e_hip = max |A - c64|     bound = CAM_BAR + FP64_FACTOR e_ref
    verdict: ok (0) if lit <= CAM_BAR; exempt (1) if cond > COND_MAX and own <= CAM_BAR and e_hip <= bound; else fail (2); a plane of A with a
    non-finite element fails; an inactive plane is ignored (-1, a row of zeros).
Everything is formed in float64 from the widened inputs, one operation per rounding in the order written; NaN never enters a maximum."""
import numpy as np

FIGS = ("d", "lit", "cond", "own", "e_ref", "e_hip", "bound", "max32")


def _nanmax0(a):
    """max over the elements that are not NaN, from 0 (what a chain of fmax from 0 gives)"""
    a = a[~np.isnan(a)]
    return float(a.max()) if a.size else 0.0


def planes(camA, cam32, cam64, active, peak64, rawmax64, cam_bar, cond_max, fp64_factor):
    """-> (fig [B, C, 8] float64 in FIGS order, verdict [B, C] int32, nonfinite [B, C] int32)"""
    camA, cam32, cam64 = np.asarray(camA, np.float32), np.asarray(cam32, np.float32), np.asarray(cam64, np.float64)
    B, C = camA.shape[:2]
    fig, vd, bad = np.zeros((B, C, len(FIGS))), np.full((B, C), -1, np.int32), np.zeros((B, C), np.int32)
    with np.errstate(all="ignore"):
        for i in range(B):
            for c in range(C):
                if active is not None and active[i, c] == 0:
                    continue
                a, c32, c64 = camA[i, c].astype(np.float64), cam32[i, c].astype(np.float64), cam64[i, c]
                peak, rawmax = np.float64(peak64[i, c]), np.float64(rawmax64[i, c])
                d, m32 = _nanmax0(np.abs(a - c32)), _nanmax0(np.abs(c32))
                e_ref, e_hip = _nanmax0(np.abs(c32 - c64)), _nanmax0(np.abs(a - c64))
                lit = np.float64(d) / max(m32, 1e-6)
                cond = rawmax / peak
                own = np.float64(d) * peak / max(rawmax, 1e-30)
                bound = np.float64(cam_bar) + np.float64(fp64_factor) * np.float64(e_ref)
                bad[i, c] = int((~np.isfinite(camA[i, c])).sum())
                if bad[i, c]:
                    v = 2
                elif lit <= cam_bar:
                    v = 0
                elif cond > cond_max and own <= cam_bar and e_hip <= bound:
                    v = 1
                else:
                    v = 2
                fig[i, c] = (d, lit, cond, own, e_ref, e_hip, bound, m32)
                vd[i, c] = v
    return fig, vd, bad


def counts(vd):
    return {"planes": int((vd >= 0).sum()), "literal_ok": int((vd == 0).sum()), "exempt": int((vd == 1).sum()), "failed": int((vd == 2).sum())}


def hand_built(S, seed=0):
    """B = 2, C = 4 planes of S x S that hit every branch, with the verdicts they must get:
      (0,0) ok   (0,1) over the bar at cond 49.9 -> fail   (0,2) cond 51, own and fp64 legs inside -> exempt   (0,3) cond 51, own over -> fail
      (1,0) cond 51, e_hip just over its bound -> fail   (1,1) the same just under -> exempt   (1,2) inactive   (1,3) a NaN element -> fail
    -> dict(camA, cam32, cam64, active, peak, rawmax, verdict)"""
    rng = np.random.default_rng(seed)
    B, C = 2, 4
    c64 = rng.random((B, C, S, S))
    c64[:, :, 0, 0], c64[:, :, -1, -1] = 0.0, 1.0
    c32 = c64.astype(np.float32)
    e_ref = np.abs(c32.astype(np.float64) - c64).reshape(B, C, -1).max(-1)
    A = c32.copy()
    peak, rawmax = np.ones((B, C)), np.full((B, C), 10.0)
    active = np.ones((B, C), np.float32)

    def bump(i, c, by, at=(1, 1)):
        """A differs from c32 in one element by `by` (an fp32 step): d = |by| up to the fp32 rounding of the sum"""
        A[i, c, at[0], at[1]] = np.float32(c32[i, c, at[0], at[1]] + np.float32(by))

    bump(0, 0, 2e-4)                                        # ok: lit ~ 2e-4
    bump(0, 1, 2e-3); rawmax[0, 1] = 49.9                   # over, cond 49.9: no exemption
    bump(0, 2, 2e-3); rawmax[0, 2] = 51.0                   # own = 2e-3 / 51 <= 1e-3 but e_hip ~ 2e-3 > 1e-3 + 4 e_ref ... unless c64 moves too:
    bump(0, 3, 6e-2); rawmax[0, 3] = 51.0                   # own = 6e-2 / 51 > 1e-3: fail
    bump(1, 0, 2e-3); rawmax[1, 0] = 51.0
    bump(1, 1, 2e-3); rawmax[1, 1] = 51.0
    active[1, 2] = 0
    bump(1, 2, 0.5)
    A[1, 3, 2, 2] = np.nan
    # the fp64 legs: put c64 itself off c32 at the bumped element, so that e_ref is large enough for the bound to admit (or just refuse) e_hip.
    # With c64 = c32 + t at that element: e_ref = t, e_hip = |by - t|, bound = 1e-3 + 4 t.
    for (i, c), t in (((0, 2), 1e-3), ((1, 0), None), ((1, 1), None)):
        a, r = np.float64(A[i, c, 1, 1]), np.float64(c32[i, c, 1, 1])
        if t is not None:
            c64[i, c, 1, 1] = r + t                         # e_hip ~ 1e-3 <= 1e-3 + 4e-3: exempt
            continue
        # e_hip = a - x, e_ref = r - x (x below both) -> e_hip - (bar + 4 e_ref) = (a - r) - 1e-3 - 3 (r - x): zero at r - x = ((a - r) - 1e-3) / 3
        gap = ((a - r) - 1e-3) / 3
        c64[i, c, 1, 1] = r - gap * (0.999 if (i, c) == (1, 0) else 1.001)          # a smaller e_ref: just over; a larger one: just under
    verdict = np.array([[0, 2, 1, 2], [2, 1, -1, 2]], np.int32)
    return dict(camA=A, cam32=c32, cam64=c64, active=active, peak=peak, rawmax=rawmax, verdict=verdict)
