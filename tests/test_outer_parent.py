"""The outer layer's unification (one rollout wave body, one drive tick, one launch path, argument structs filled
once) changes no arithmetic: on the host build every output of the rollouts, the PID drives, the fused segment
times and one call each of the tyre fit, the tyre loss / gradient and the GA's breeding stays bitwise equal to the
recording made with the libraries of the commit before it (tests/golden/outer_parent.npz, generator
tests/golden/make_outer_parent_golden.py).  tests/test_gpu_outer_parent.py is the same on gfx950."""
import importlib.util
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_ARRAYS = 117  # 8 rollouts x 6, 6 drives x 4, 6 drives without rows x 3, 6 segment runs x 2, 7 + 2 + 6 single calls


def generator():
    spec = importlib.util.spec_from_file_location("make_outer_parent_golden",
                                                  os.path.join(GOLDEN, "make_outer_parent_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check_bitwise_equal_to_parent(backend):
    with np.load(os.path.join(GOLDEN, "outer_parent.npz")) as z:
        golden = {k[len(backend) + 1:]: z[k] for k in z.files if k.startswith(backend + "/")}
    out = generator().record(backend)
    assert sorted(out) == sorted(golden) and len(golden) == N_ARRAYS
    bad = []
    for k, g in golden.items():
        a = np.ascontiguousarray(out[k])
        assert a.dtype == g.dtype and a.shape == g.shape, k
        if not np.array_equal(a.view(np.uint8), g.view(np.uint8)):  # bitwise: NaNs and infs must match too
            bad.append(k)
    assert not bad, bad


def test_host_outputs_bitwise_equal_to_parent():
    check_bitwise_equal_to_parent("host")
