"""Record tests/golden/closed_loop_blend_golden.npz: three ticks of ``ClosedLoop(plant="blend")`` for four
vehicles, as computed on an MI355X by the library of the commit BEFORE the learned plant was added
(``--package-root`` names that commit's ``mpc-racing_amd``).  tests/test_gpu_rollout.py holds the same setup
(``run_blend`` below) bitwise equal to the recording: adding ``plant="learned"`` changed no other plant path.
Recorded again when the fp64 Riccati sweep's cost-to-go tile was made symmetric (mr_wave.h frag_plan):
the loop's fp64 MPC solves (tol 1e-10) moved in their last bits on purpose, nothing of the plant did.

TEST FIXTURE GENERATOR (needs the GPU; run once per change of the setup).

Usage: python tests/golden/make_blend_loop_golden.py [--package-root <mpc-racing_amd of the recording commit>]
       [--out tests/golden/closed_loop_blend_golden.npz]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("X", "Y", "yaw", "vx", "vy", "yawdot", "progress", "error", "cmd_throttle", "cmd_steer", "cmd_brake",
        "status", "iters", "controls", "predicted_states")
S0, V0, OFFSET, TICKS = (120.0, 800.0, 1500.0, 2600.0), 14.0, 0.3, 3


def make_loop(ClosedLoop, plant, **kw):
    """The loop of both the recording and the tests: B = 4, N = 15, MPC from the second tick on."""
    loop = ClosedLoop("shanghai_intl_circuit", B=len(S0), N=15, plant=plant, start_control_at=1, tol=1e-10,
                      acceptable_iter=0, **kw)
    loop.reset(ClosedLoop.start_states(loop.track, np.array(S0), v0=V0, offset=OFFSET))
    return loop


def run_blend(ClosedLoop):
    import torch
    loop = make_loop(ClosedLoop, "blend")
    recs = loop.run(TICKS)
    torch.cuda.synchronize()
    out = {"state": loop.state.cpu().numpy()}
    for t, r in enumerate(recs):
        for k in KEYS:
            if r[k] is not None:
                out[f"tick{t}/{k}"] = r[k].cpu().numpy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(HERE, "..", "..", "mpc-racing_amd")))
    ap.add_argument("--out", default=os.path.join(HERE, "closed_loop_blend_golden.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    from mpcracing import abi
    from mpcracing.closed_loop import ClosedLoop
    out = run_blend(ClosedLoop)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(f"library {abi.PRODUCT_LIB}: {len(out)} arrays -> {a.out}")


if __name__ == "__main__":
    main()
