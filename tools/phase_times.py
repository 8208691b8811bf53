"""Per-phase shader-clock breakdown of k_disc_chain4 / k_disc_chain and a wall-clock timeline of chain -> k_disc_wgrad, in the
two-launch, ungraphed form (the stamped build never runs k_disc_step4 or the replayed graph).
Needs the disc_stamps variant of BOTH libraries (bash tools/build_variant.sh disc_stamps "" tools/diag/disc_stamps.patch) in place
of simgan_amd/libsimgan_hip.so and simgan_amd/libsimgan_hip_test.so -- in a copy of the tree; run on the GPU box:
python tools/phase_times.py [workload]"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd import _lib  # noqa: E402
from bench import WORKLOADS, build_problem  # noqa: E402

w = WORKLOADS[sys.argv[1] if len(sys.argv) > 1 else "northstar"]
pol, disc, agent, ro, loader, expert, learner = build_problem(sg, w, 0)
lib = _lib.load()
_lib.check(lib.sg_rollout_fill_synthetic(ro.h, pol.h, 1234, 0.01))
# the hook exists in the disc_stamps variant only, so it is bound here and not through _lib.TEST_PROTOTYPES (the in-tree test library's table)
tlib = C.CDLL(_lib.TEST_LIB_PATH)
if not hasattr(tlib, "sg_test_disc_phase_times"):
    sys.exit(f"{_lib.TEST_LIB_PATH} has no sg_test_disc_phase_times: build the disc_stamps variant (see tools/README.md)")
tlib.sg_test_disc_phase_times.restype = C.c_int
tlib.sg_test_disc_phase_times.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.c_int]
tlib.sg_test_last_error.restype = C.c_char_p
ROWS, WG = 512, 512   # SG_DISC_STAMP_ROWS chain workgroups of 32 stamps, then SG_DISC_STAMP_WG k_disc_wgrad workgroups of 4 (the patch's sg_common.h)


def fn(*args):
    if tlib.sg_test_disc_phase_times(*args) != 0:
        raise RuntimeError(tlib.sg_test_last_error().decode(errors="replace"))


disc.update_gail_dyn(loader, ro)  # warm
fn(disc.h, 1, None, 0)
disc.update_gail_dyn(loader, ro)
thin = os.environ.get("SG_DISC_CHAIN", "thin") != "wide"
nb = (12 if thin else 2) * ((w["B"] + 15) // 16)
assert nb <= ROWS, f"{nb} chain workgroups, the stamp buffer holds {ROWS}"
full = (C.c_longlong * (32 * ROWS + 4 * WG))()
fn(disc.h, 1, full, len(full))
f = np.array(full, dtype=np.int64)
t = f[: 32 * nb].reshape(nb, 32)
for name, b in ((("mix block 0", 0), ("mix block 9", 9), ("BCE block", nb // 3 + 5)) if thin else (("BCE block 0", 0), ("mix block", nb // 2))):
    row = t[b]
    idx = sorted([i for i in range(32) if row[i] != 0 and i not in (28, 29)], key=lambda i: row[i])
    print(name, "total cycles", row[idx[-1]] - row[idx[0]])
    for i0, i1 in zip(idx[:-1], idx[1:]):
        print(f"   phase {i0:2d}->{i1:2d}: {row[i1] - row[i0]:8d} cycles")
# wall-clock (100 MHz) timeline of the LAST step of the epoch: chain blocks, then k_disc_wgrad blocks by role
cs, ce = t[:, 28], t[:, 29]
t0 = cs.min()
print(f"chain: blocks start {10 * (cs.min() - t0)}..{10 * (cs.max() - t0)} ns, end {10 * (ce.min() - t0)}..{10 * (ce.max() - t0)} ns")
wg = f[32 * ROWS:].reshape(WG, 4)
G = (w["B"] + 15) // 16
kf, kh = (w["F"] + 15) // 16, (w["Hd"] + 15) // 16
nt, nv = kh * kh + kh * kf, (3 * 16 * kh + 4 + 63) // 64
st = wg[:, 0]
live = st[st > 0]
print(f"wgrad: all blocks start {10 * (live.min() - t0)}..{10 * (live.max() - t0)} ns after the chain's first block")
tl = wg[wg[:, 1] > 0]     # tile blocks are the ones that stamp their load / reduce / store points
for nm, k in (("operands loaded + MFMA", 1), ("LDS reduce barrier", 2), ("Adam + stores issued", 3)):
    dt = 10 * (tl[:, k] - tl[:, 0])
    print(f"wgrad tiles: {nm:24s} at +{dt.min()}..{dt.max()} ns (median {int(np.median(dt))})")
sp = wg[(wg[:, 1] == 0) & (wg[:, 3] > 0)]
if len(sp):
    print(f"wgrad Adam-scalar lane (double pow): done at +{10 * int((sp[:, 3] - sp[:, 0]).max())} ns")
fn(disc.h, 0, None, 0)
