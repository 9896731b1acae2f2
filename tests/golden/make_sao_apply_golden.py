"""Generates tests/golden/sao_apply_golden.npz: outputs of the REFERENCE's own in-loop SAO (turing/LoopFilter.h's LoopFilter::Picture in
the encoder's form, TaskSao.cpp:96-121, over tests/sao_apply_shim.cpp) on the seeded pictures of tests/sao_apply_tools.py.  Each plane is
stored as its difference from the deblocked input (int16), which is zero almost everywhere.
python tests/golden/make_sao_apply_golden.py  (byte-identical on rerun)"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import sao_apply_tools as A      # noqa: E402

SEEDS = range(900, 936)


def main():
    shim = A.Shim()
    arrays = {}
    for s in SEEDS:
        pic = A.make_picture(s)
        enc, dec = shim.picture(pic)
        for k, o, r in zip(("y", "cb", "cr"), enc, (pic["rec_y"], pic["rec_cb"], pic["rec_cr"])):
            assert np.array_equal(o, dec[("y", "cb", "cr").index(k)])
            arrays[f"{k}{s}"] = (o.astype(np.int32) - r.astype(np.int32)).astype(np.int16)
    path = os.path.join(HERE, "sao_apply_golden.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:      # fixed member dates: the file is byte-identical on every run
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED)
    print("wrote", len(arrays), "arrays")


if __name__ == "__main__":
    main()
