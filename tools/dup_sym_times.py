"""Milliseconds of sg_rollout_dup_sym (one launch that makes the mirrored half of a 2n-column rollout on the device) and of
what it replaces: uploading the mirrored half of every field from page-locked host memory.  Device timestamps
(sg_ctx_mark), medians over 20 repetitions, both in one process, at T = 128, n = 256 with (O, A) = (47, 12) and (111, 12);
the feature slot carries the observation, as driver.PpoLearner fills it.

The replaced upload is timed as sg_rollout_upload_columns of n columns per field: the same bytes in the same strided shape
as columns [n, 2n) of the page-locked host tensors, one copy per field.  Also recorded: the whole-width upload of every
field that a driver mirroring on the host pays per rollout.
Run on the GPU box:  python tools/dup_sym_times.py [--json PATH]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd import _lib  # noqa: E402

REPS = 20
DUP_FIELDS = (_lib.F_OBS, _lib.F_OBS_FEAT, _lib.F_ACTIONS, _lib.F_REWARDS, _lib.F_VALUE_PREDS, _lib.F_LOGP, _lib.F_MASKS, _lib.F_BAD_MASKS)


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def dense_like_laikago(w, rng):
    """A signed permutation with a few mixing blocks: the sparsity of the Laikago mirrors at any width."""
    m = np.zeros((w, w), np.float32)
    m[np.arange(w), rng.permutation(w)] = rng.choice([-1.0, 1.0], w)
    m[:3, :3] = rng.standard_normal((3, 3))
    return m


def median_ms(ctx, fn, reps=REPS, warmup=3):
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    ms = []
    for _ in range(reps):
        a = ctx.mark()
        fn()
        b = ctx.mark()
        ms.append(ctx.mark_elapsed(a, b))
    ctx.marks_reset()
    return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4), round(float(np.max(ms)), 4)


def time_shape(T, n, O, A):
    rng = np.random.default_rng(O)
    ro = sg.RolloutStorage(T, 2 * n, (O,), Box((A,)), 1, O)
    ctx, lib = ro.ctx, ro.lib
    for f in DUP_FIELDS:
        a = ro._host_np(f)
        a[...] = rng.standard_normal(a.shape).astype(np.float32)
    ro.device_resident = True
    if O % 37 == 0:
        from simgan_amd.symmetry import laikago_mirror
        m_obs, _ = laikago_mirror(O)
    else:
        m_obs = dense_like_laikago(O, rng)
    m_act = dense_like_laikago(A, rng)
    ro.enable_dup_sym(m_obs, m_act)
    host = {f: ro._host_np(f) for f in DUP_FIELDS}

    def half_upload():
        for f, a in host.items():
            _lib.check(lib.sg_rollout_upload_columns(ro.h, f, n, _lib.fptr(a), a.size))

    def full_upload():
        for f, a in host.items():
            _lib.check(lib.sg_rollout_upload(ro.h, f, _lib.fptr(a), a.size))

    out = {"T": T, "n": n, "O": O, "A": A, "feat_len": O, "reps": REPS,
           "mirrored_half_bytes": int(sum(a.nbytes // 2 for a in host.values()))}
    for name, fn in (("dup_sym_kernel", lambda: _lib.check(lib.sg_rollout_dup_sym(ro.h))), ("mirrored_half_upload", half_upload),
                     ("full_width_upload", full_upload)):
        med, lo, hi = median_ms(ctx, fn)
        out[name] = {"ms_median": med, "ms_min": lo, "ms_max": hi}
    out["kernel_over_half_upload"] = round(out["dup_sym_kernel"]["ms_median"] / out["mirrored_half_upload"]["ms_median"], 4)
    return out


def main():
    res = {"what": "device-timestamp medians (sg_ctx_mark), one process", "shapes": [time_shape(128, 256, 47, 12), time_shape(128, 256, 111, 12)]}
    for s in res["shapes"]:
        print(s, flush=True)
    print(json.dumps(res))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
