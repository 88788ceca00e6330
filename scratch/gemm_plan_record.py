#!/usr/bin/env python3
"""Records tests/golden/gemm_plans.txt from the launcher as it was BEFORE gemm.hip was split into plan and execute.

    git worktree add /tmp/parent <the commit in front of the split>      (any checkout of that commit outside this tree)
    (cd /tmp/parent && git apply <this tree>/scratch/gemm_plan_parent.patch && bash ast_amd/csrc/build.sh)
    python3 scratch/gemm_plan_record.py /tmp/parent/ast_amd/libastk_test.so [OUT]

The patch puts astk_debug_gemm_plan on top of the old gemm_launch_group: made-up 16-byte aligned operand addresses, the decisions written
to the caller's buffer, return in front of the first device call.  The case table is the test's own (tests/test_gemm_plan_host.py), so
recorder and test cannot drift apart.  Not a test, and no test runs it.  Refuses to run where a GPU is visible: the addresses are made
up, and a library without the patch's early return would launch on them.
With the library of THIS tree (ast_amd/libastk_test.so) the output must equal the golden file: that is what the test checks."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_visible():
    if os.path.exists("/dev/kfd"):
        return True
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def main():
    if gpu_visible():
        sys.exit("gemm_plan_record.py: a GPU is visible here; record on a machine without one")
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import test_gemm_plan_host as T
    from ast_amd import _lib
    lib = C.CDLL(os.path.abspath(sys.argv[1]))
    for name in ("astk_debug_gemm_plan", "astk_get_tuning", "astk_set_tuning", "astk_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = (_lib.TEST_HOOK_SIGNATURES if name in _lib.TEST_HOOK_SIGNATURES else _lib.SIGNATURES)[name]
    out = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
    with open(out, "w") as f:
        for c in T.CASES:
            f.write(f"# {c['name']}\n{T.plan_text(lib, c)}")
    print(f"{len(T.CASES)} cases -> {out}")


if __name__ == "__main__":
    main()
