"""Generates tests/golden/deblock_golden.npz: outputs of the REFERENCE's own deblocking (turing/LoopFilter.h's
LoopFilter::Picture::deblock<EDGE_VER / EDGE_HOR> templates in its CTU order, oracle/ref_shim_deblock.cpp in oracle/_ref/libhavoc_ref.so)
on the seeded pictures of tests/deblock_tools.py.  Each plane is stored as its difference from the input (int16).
python tests/golden/make_deblock_golden.py  (byte-identical on rerun)"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import deblock_tools as D      # noqa: E402
import reflibs                 # noqa: E402

SEEDS = range(900, 936)


def main():
    ref = reflibs.Reference(0)
    arrays, depths = {}, set()
    for s in SEEDS:
        pic = D.make_picture(s)
        depths.add((pic["bd"], pic["S"]))
        for k, o in zip(("y", "cb", "cr"), D.run_cpu(ref, pic)):
            arrays[f"{k}{s}"] = (o.astype(np.int32) - pic[k].astype(np.int32)).astype(np.int16)
    assert depths == {(8, 1), (8, 2), (9, 2), (10, 2)}, depths
    path = os.path.join(HERE, "deblock_golden.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:      # fixed member dates: the file is byte-identical on every run
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED)
    print("wrote", len(arrays), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
