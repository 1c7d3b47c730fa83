"""The selection of a focused progressive step, restated in NumPy: the normative definition
(include/rt_amd.h restates it in words; csrc/focus.hip computes it on the device).

    score      one fp32 per pixel; not (>= 0 and finite) -> 0
    eligible   active pixels with score > min_score
    K          (n_active * permille + 999) // 1000, capped by max_pixels when > 0
    T          the K-th largest eligible score, compared as the uint32 bit pattern (which orders
               non-negative finite floats); the smallest eligible one when at most K are eligible
    selected   the eligible pixels with score >= T: ties at T are all taken
"""
import numpy as np


def sanitise(score):
    s = np.asarray(score, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where((s >= 0) & np.isfinite(s), s, np.float32(0)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def select(score, active, permille=250, min_score=0.0, max_pixels=0):
    """score: float array of any shape; active: bool array of the same shape (the pixels still
    sampling). Returns {"mask": bool array, "threshold": np.float32 (0 when nothing is eligible),
    "active", "eligible", "selected", "k": ints}."""
    s = sanitise(score)
    active = np.asarray(active, bool)
    assert s.shape == active.shape
    b = bits(s).astype(np.int64)                      # (-0 has become +0 or stays ineligible: see below)
    b[b >= 0x80000000] = 0                            # -0.0 passes "s >= 0"; it is never > min_score
    mb = int(bits(np.float32(min_score)).reshape(())[()]) if min_score != 0 else 0
    eligible = active & (b > mb)
    n_active = int(active.sum())
    k = (n_active * int(permille) + 999) // 1000
    if max_pixels > 0:
        k = min(k, int(max_pixels))
    e = np.sort(b[eligible])[::-1]                    # the eligible bit patterns, largest first
    if e.size == 0:
        return {"mask": np.zeros(s.shape, bool), "threshold": np.float32(0), "active": n_active, "eligible": 0,
                "selected": 0, "k": k}
    t = int(e[min(k, e.size) - 1])
    mask = eligible & (b >= t)
    return {"mask": mask, "threshold": np.array([t], np.uint32).view(np.float32)[0], "active": n_active,
            "eligible": int(e.size), "selected": int(mask.sum()), "k": k}
