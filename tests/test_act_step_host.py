"""CPU: utils.step_masks, the masks / bad_masks helper of both collection paths, against the expressions it replaced
(a2c/main_gail_dyn_ppo.py:228-231, a2c/main.py:226-229) on random `done` / `infos`."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def reference_masks(done, infos):
    """The list comprehensions of the collection loops, as they stood."""
    masks = np.array([[0.0] if d else [1.0] for d in done], np.float32)
    bad = np.array([[0.0] if 'bad_transition' in info.keys() else [1.0] for info in infos], np.float32)
    return masks, bad


def same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("N", [1, 2, 17, 512])
@pytest.mark.parametrize("done_kind", ["bool_array", "list", "float_array", "int_array"])
def test_step_masks_equals_the_loops(N, done_kind):
    from simgan_amd.utils import step_masks
    rng = np.random.default_rng(N)
    for trial in range(5):
        d = rng.random(N) < (0.0, 0.3, 0.5, 1.0, 0.1)[trial]
        done = {"bool_array": d, "list": [bool(x) for x in d], "float_array": d.astype(np.float32) * 2.5,
                "int_array": d.astype(np.int64)}[done_kind]
        infos = []
        for i in range(N):
            k = rng.integers(0, 4)
            infos.append([{}, {"bad_transition": True}, {"bad_transition": False, "x": 1}, {"episode": {"r": 1.0}}][k])
        infos[rng.integers(0, N)] = {}     # an info without keys
        want, got = reference_masks(done, infos), step_masks(done, infos)
        assert same(got[0], want[0]) and same(got[1], want[1])
        assert got[0].shape == (N, 1) and got[1].shape == (N, 1)


def test_step_masks_takes_a_tuple_of_infos_and_mapping_likes():
    from simgan_amd.utils import step_masks

    class Info:   # anything with keys(), as the loops asked
        def __init__(self, ks):
            self.ks = ks

        def keys(self):
            return self.ks

    infos = (Info(["bad_transition"]), Info([]), Info(["a", "bad_transition"]))
    done = (True, False, False)
    want, got = reference_masks(done, infos), step_masks(done, infos)
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert got[1][:, 0].tolist() == [0.0, 1.0, 0.0] and got[0][:, 0].tolist() == [0.0, 1.0, 1.0]
