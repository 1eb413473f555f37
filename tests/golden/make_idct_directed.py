"""Generate tests/golden/idct_directed.npz: the witness vectors of tests/directed_idct.py (seeded
search) run through the REAL reference transform.

Needs oracle/_ref/ref_kernels (`make -C oracle ref`).  Every vector (F, flat pred) goes through
inverse_dct_template<false> and <true> (idct_sse2.hpp:96-120); the file holds F, pred, the
reference's put and add, each vector's form (0: a put witness, 1: an add witness) and the search's
record: names, conds (mutant, form, line or -1, vector) and bounded (mutant, form, line).
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import directed_idct as I  # noqa: E402
from gen_kernel_vectors import REF_KERNELS, run_idct  # noqa: E402


def main():
    if not os.path.exists(REF_KERNELS):
        sys.exit("build the reference first: make -C oracle ref")
    V = I.search()
    assert not V.unkilled, V.unkilled
    pred = V.pred()
    cF = np.array([I.corner_qfs(kind, words) for kind, words in I.corner_blocks()], np.int16)
    cpred = np.full((len(cF), 64), 128, np.uint8)
    cpred[1::3], cpred[2::3] = 0, 255
    with tempfile.TemporaryDirectory() as tmp:
        put, add = run_idct(V.F, pred, tmp)
        cput, cadd = run_idct(cF, cpred, tmp)
    idx = {n: i for i, n in enumerate(I.NAMES)}
    np.savez_compressed(I.FIXTURE, corner_F=cF, corner_pred=cpred, corner_put=cput, corner_add=cadd,
                        F=V.F, pred=pred, form=V.form, put=put, add=add, names=np.array(I.NAMES),
                        conds=np.array([(idx[n], f, ln, v) for n, f, ln, v in V.conds], np.int16),
                        bounded=np.array([(idx[n], f, ln) for n, f, ln in V.bounded], np.int16))
    print("vectors", len(V.F), "conditions", len(V.conds), "bounded", len(V.bounded),
          "bytes", os.path.getsize(I.FIXTURE))


if __name__ == "__main__":
    main()
