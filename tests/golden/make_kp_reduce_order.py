"""Records tests/golden/kp_reduce_order/*.npz for tests/test_gpu_kp_reduce_order.py.

Run on a GPU with PLSSVM_MI_LIB naming the library of the commit BEFORE the slab pass was reshaped (5202d1c): the
fixtures pin that build's summation order, so they must never be recorded from the build under test.

    PLSSVM_MI_LIB=/path/to/parent/libplssvm_mi355x.so python tests/golden/make_kp_reduce_order.py

Every K·p is taken with the tile cache on and off, computed and streamed, and the CG both ways; the script refuses to
write a fixture when those disagree (they are bitwise equal in that build).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_gpu_kp_reduce_order as t  # noqa: E402


def kp(kernel, dtype, m, sim=None):
    outs = t.kp_twice(kernel, dtype, m, True, sim)[0] + t.kp_twice(kernel, dtype, m, False, sim)[0]
    for o in outs[1:]:
        assert np.array_equal(o, outs[0]), (kernel, dtype, m, sim)
    assert np.isfinite(outs[0]).all()
    np.savez_compressed(os.path.join(t.GOLDEN, t.kp_name(kernel, dtype, m, sim) + ".npz"), kp=outs[0])


def main():
    assert os.environ.get("PLSSVM_MI_LIB"), "record from the parent build: set PLSSVM_MI_LIB"
    os.makedirs(t.GOLDEN, exist_ok=True)
    for kernel in t.KERNELS:
        for dtype in t.DTYPES:
            for m in t.SHAPES:
                kp(kernel, dtype, m)
    for sim in t.SIMS:
        kp("rbf", "f64", t.M_SIM, sim)
    x, trace = t.cg60(False)
    x1, trace1 = t.cg60(True)
    assert np.array_equal(x, x1) and np.array_equal(trace, trace1)
    np.savez_compressed(os.path.join(t.GOLDEN, "cg_rbf_f64_1100.npz"), x=x, trace=trace)
    total = sum(os.path.getsize(os.path.join(t.GOLDEN, f)) for f in os.listdir(t.GOLDEN))
    print(f"wrote {len(os.listdir(t.GOLDEN))} fixtures, {total} bytes")


if __name__ == "__main__":
    main()
