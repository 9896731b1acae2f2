"""Generates tests/golden/sao_merge_golden.npz: outputs of the REFERENCE's own SAO decision (turing/EncSao.h rdSao with its estimates and
Search<sao>::go, over tests/sao_merge_shim.cpp) on the seeded pictures of tests/sao_merge_tools.py, chroma statistics where the reference
reads them.  Pictures where a band search starts at position 29 (the reference reads past its band arrays there) are skipped.  Records
are stored as the reference holds them (stale fields of type-0 components); sao_merge_tools.normalise_shim gives the device's form.
python tests/golden/make_sao_merge_golden.py  (byte-identical on rerun)"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import reflibs                   # noqa: E402
import sao_merge_tools as M      # noqa: E402

N = 30          # pictures
FIRST = 600     # first seed tried


def seeds(oracle):
    """the first N seeds from FIRST whose band searches never start at position 29"""
    out, s = [], FIRST
    while len(out) < N:
        und = []
        M.decide_picture(oracle, M.make_picture(s), chroma_stats="reference", undefined=und)
        if not np.array(und).any():
            out.append(s)
        s += 1
    return out


def main():
    shim, oracle = M.Shim(), reflibs.Oracle()
    arrays = {}
    for s in seeds(oracle):
        rec, dy, dc = shim.picture(M.make_picture(s))
        arrays[f"rec{s}"], arrays[f"dst_y{s}"], arrays[f"dst_c{s}"] = rec, dy, dc
    path = os.path.join(HERE, "sao_merge_golden.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:      # fixed member dates: the file is byte-identical on every run
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED)
    print("wrote", len(arrays), "arrays")


if __name__ == "__main__":
    main()
