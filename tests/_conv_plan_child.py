"""Child process of tests/test_conv_plans.py::test_64bit_addressed_kernel_on_every_tile: PCC_CONV_PATH is read once per
process, so the 64-bit-addressed kernel (conv_mfma_kernel) is forced in a process of its own.  Runs GLOBAL_CASES — the fp32
table at one even and one odd chunk count per tile, with a map and without — against the chain oracle, stops at the first
mismatch (exit status 1, the case named) and prints `RAN <count>` at the end."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def main():
    import pcc_amd
    import _conv_plan_cases as cp
    assert os.environ.get("PCC_CONV_PATH") == "global"
    L = pcc_amd.lib()
    t0 = time.time()
    ran = 0
    for case in cp.GLOBAL_CASES:
        with cp.small_threshold(L, case.small):
            name = cp.case_name(L, case)
        if not (isinstance(name, str) and name.startswith("conv_mfma_kernel<")):
            print(f"FAILED {case.id}: planned {name}, not the 64-bit-addressed kernel", flush=True)
            return 1
        try:
            cp.run_case(pcc_amd, case, forms=("null", "permutation"), with_float64=False, with_sub_rows=False)
        except AssertionError as e:
            print(f"FAILED {case.id}: {e}", flush=True)
            return 1
        ran += 1
        print(f"OK {case.id} {name}", flush=True)
    print(f"RAN {ran} in {time.time() - t0:.1f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
