"""Generator of tests/golden/soc_trace_parent.npz (tests/test_gpu_soc_trace_golden.py).

The full iteration trace, every output array and lam_g of six single-instance GPU solves, recorded with the
product library of the commit *before* the lean second-order correction (constants staged in LDS, the dual side
finished by soc_commit), which changes no arithmetic: everything must stay bitwise equal.  Unlike the final
outputs alone, the trace shows a changed last bit of the dual step size or of a dual step in the iteration it
happens (column 2, alpha, and column 0, the KKT error of the next iterate).  Run on the GPU from the repository
root:

    python tests/golden/make_soc_trace_golden.py [OUT.npz]

Cases (keys "<case>/<array>"), each solved alone (B = 1) with trace_instance 0, trace_cap 560, duals:
  C4_4341, C4_2586, C4_3049   fp32: the shard's long solves (hundreds of corrections, most of them rejected)
  C3_123, C3_321              fp64, lane rows: at least 5 accepted corrections each (asserted when recording;
                              123 converges in 117 iterations with 5, 321 runs to max_iter with 16 in the host
                              wave build).  321 replaces 326, which ran to max_iter with 26 until the Riccati
                              sweep's cost-to-go tile was made symmetric (mr_wave.h frag_plan) and takes none since
  C3_21                       fp64: of the shard's first 32 instances none has 5 accepted corrections at the
                              product's fp64 options (a scan with the recording library: 21 has 3, 1 / 10 / 17
                              have 1, the others none), so the first with 5 is taken from further on (123) and
                              the first 32's best is recorded as well (at least 3 asserted)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "mpc-racing_amd"))

TRACE_CAP = 560
CASES = {
    "C4_4341": ("C4", "fp32", 4341),
    "C4_2586": ("C4", "fp32", 2586),
    "C4_3049": ("C4", "fp32", 3049),
    "C3_123": ("C3", "fp64", 123),
    "C3_321": ("C3", "fp64", 321),
    "C3_21": ("C3", "fp64", 21),
}
C3_MIN_ACCEPTED = {"C3_123": 5, "C3_321": 5, "C3_21": 3}


def solve_case(case):
    """Every output of the case's solve as numpy arrays (trace and lam_g among them)."""
    from mpcracing import workload as wl
    from mpcracing.batch import solver_for_config
    name, precision, i = CASES[case]
    b = wl.make_batch(name, limit=i + 1)
    sub = {k: (np.ascontiguousarray(v[..., i:i + 1]) if v is not None else None) for k, v in b.items()}
    out = solver_for_config(name, 1, precision=precision).solve(sub, trace_instance=0, trace_cap=TRACE_CAP,
                                                                duals=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


def accepted_corrections(out):
    """Iterations of the trace whose step is an accepted second-order correction (marker >= 100)."""
    n = int(out["iters"][0])
    return int((out["trace"][:min(n, TRACE_CAP - 2), 7] >= 100).sum())


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "soc_trace_parent.npz")
    arrays = {}
    for case in CASES:
        out = solve_case(case)
        again = solve_case(case)
        for k, v in out.items():  # a recording is only worth comparing against if the solve repeats itself
            assert np.array_equal(v.view(np.uint8), again[k].view(np.uint8)), (case, k)
            arrays[f"{case}/{k}"] = v
        nacc = accepted_corrections(out)
        if case in C3_MIN_ACCEPTED:
            assert nacc >= C3_MIN_ACCEPTED[case], (case, nacc)
        print(case, "iters", int(out["iters"][0]), "status", int(out["status"][0]), "accepted corrections", nacc,
              flush=True)
    np.savez_compressed(dst, **arrays)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
