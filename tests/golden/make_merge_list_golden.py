"""Generates tests/golden/merge_list_golden.npz: a sample of the merge candidate lists the traced REFERENCE encoder left (the HAVOC_TRACE_MERGE trace point, obtained as
tests/test_trace_pin.py obtains it: trace_tools.run + trace_tools.MergeTrace over the six traced encodes), for tests/test_merge_list.py to hold
turingcodec_amd/search/merge_list.hpp against where the traced encoder is absent.  Data only: `rows` int32 [m, 64] = the inputs in tests/search_client.cpp:
client_merge's layout (partIdx, nPbW, nPbH, sliceB, numRef0, numRef1, maxCand, colAvailable | five neighbours A1, B1, B0, A0, B2 and the temporal candidate, each
predFlag0, predFlag1, refIdx0, refIdx1, mv0 x, y, mv1 x, y | poc0[4] | poc1[4]) and `lists` int16 [m, 5, 8] = the list populateMergeCandidates left, per candidate the
same eight numbers.  The records are deduplicated; those with a pruned neighbour, a temporal candidate or a combined candidate are taken first, the rest is a seeded
random sample, and the whole is capped so that the file stays below 300 KB.  Needs the traced encoder (oracle/_ref/turing_ref_trace):
python tests/golden/make_merge_list_golden.py"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import trace_tools as tt   # noqa: E402

CASES = ("ra_medium_qp32", "ra_fast_qp32", "ra_medium_10bit_qp27", "ra_slow_qp27", "ra_medium_internal10", "ra_medium_qp22")
CAP = 300 * 1000
PATH = os.path.join(HERE, "merge_list_golden.npz")


def classes(rows, lists):
    """-> three bool [n]: a neighbour was pruned, the temporal candidate is there, a combined candidate is in the list (bi-predictive beyond what was fetched)"""
    nb = rows[:, 8:48].reshape(-1, 5, 8)
    avail = (nb[:, :, 0] != 0) | (nb[:, :, 1] != 0)
    distinct = np.array([len({tuple(x) for x, a in zip(n, av) if a}) for n, av in zip(nb, avail)])
    pruned = avail.sum(axis=1) > distinct
    fetched = np.concatenate([nb, rows[:, 48:56].reshape(-1, 1, 8)], axis=1)
    combined = np.zeros(len(rows), bool)
    for i, (lst, f) in enumerate(zip(lists, fetched)):
        have = {tuple(x) for x in f}
        combined[i] = any(c[0] and c[1] and (c[4:8] != 0).any() and tuple(c) not in have for c in lst)
    return pruned, rows[:, 7] != 0, combined


def main():
    rows, lists = [], []
    for case in CASES:
        with tempfile.TemporaryDirectory() as work:
            _, records, _, _ = tt.run(case, work, 1)
        m = tt.MergeTrace(records)
        print(case, len(m), "lists")
        rows.append(m.rows)
        lists.append(m.out)
    rows, lists = np.concatenate(rows), np.concatenate(lists)
    total = len(rows)
    assert np.abs(lists).max() < 32768
    both = np.unique(np.concatenate([rows, lists.reshape(total, 40)], axis=1), axis=0)
    rows, lists = both[:, :64].copy(), both[:, 64:].reshape(-1, 5, 8).copy()
    pruned, temporal, combined = classes(rows, lists)
    rng = np.random.default_rng(12)
    weight = pruned.astype(int) + temporal + 2 * combined
    order = np.lexsort((rng.random(len(rows)), -weight))      # the heaviest first, ties in a seeded random order
    keep = len(order)
    while True:
        sel = np.sort(order[:keep])
        np.savez_compressed(PATH, rows=rows[sel], lists=lists[sel].astype(np.int16))
        size = os.path.getsize(PATH)
        if size <= CAP:
            break
        keep = int(keep * min(0.95, CAP / size))
    print("traced", total, "distinct", len(rows), "kept", keep, "pruned", int(pruned[sel].sum()), "temporal", int(temporal[sel].sum()), "combined", int(combined[sel].sum()),
          "bytes", size)


if __name__ == "__main__":
    main()
