"""Child process of tests/test_wgrad_plans.py::test_switched_kernels_in_a_child: the A/B switches of the weight-gradient
kernels (PCC_WGRAD_SLICE, PCC_WGRAD_SLICE_O, PCC_WGRAD_AHEAD, PCC_WGRAD_BF16_SLICE_O) are read once per process, so every
launchable kernel instance but the defaults runs in a process of its own.  argv: the fp32 and the bf16 kernel the process was
started for.  Runs `child_cases(env)` against the exact references, stops at the first mismatch (exit status 1, the case
named), prints `OK <case> <kernel>` per case and `RAN <count>` at the end."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def main():
    import pcc_amd
    import _wgrad_plan_cases as wc
    env = wc.Env(*(int(os.environ[k]) for k in ("PCC_WGRAD_SLICE", "PCC_WGRAD_SLICE_O", "PCC_WGRAD_AHEAD", "PCC_WGRAD_BF16_SLICE_O")))
    want_f32, want_bf16 = sys.argv[1], sys.argv[2]
    L = pcc_amd.lib()
    t0 = time.time()
    ran = 0
    for case in wc.child_cases(env):
        plan = wc.planned(L, case.bf16, case.K, case.cin, case.cout, case.n_out)
        if not (isinstance(plan, tuple) and plan[0] == (want_bf16 if case.bf16 else want_f32)):
            print(f"FAILED {case.id}: planned {plan}, not {want_bf16 if case.bf16 else want_f32}", flush=True)
            return 1
        try:
            wc.run_case(pcc_amd, case, O=(env.bf16_O or 5) if case.bf16 else env.O)
        except AssertionError as e:
            print(f"FAILED {case.id}: {e}", flush=True)
            return 1
        ran += 1
        print(f"OK {case.id} {plan[0]}", flush=True)
    print(f"RAN {ran} in {time.time() - t0:.1f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
