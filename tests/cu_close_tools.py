"""Closing an inter coding unit -- Search<IfCbf<rqt_root_cbf, transform_tree>>::go (turing/Search.hpp:2362-2568) over Syntax<coding_unit> (turing/SyntaxCtu.hpp:143-264)
-- restated on the CPU in plain Python, in the reference's order, with the branch it takes counted by name in `tags` (a collections.Counter).  Test infrastructure.

Rates are integers (Cost = FixedPoint<int64_t, 16>): a context-coded bin costs measureEncodeDecision (sao_merge_tools.bin_cost: the tables of
turingcodec_amd/csrc/cabac_tables.h, which the device uses too) and moves its context, a bypass bin 1 << 16.  `Shim` compiles tests/cu_close_shim.cpp -- the reference's
own Syntax<coding_unit>::go and writers over a stand-in handle, and the close's cost arithmetic with the reference's Cost and Lambda -- into a temporary directory;
`DecisionClient` compiles tests/cu_close_client.cpp (search/cu_decision.hpp's closeInterCu).  `make_cases` makes the inputs of one launch of havoc_mi355x_cu_close as
a dict of arrays: a systematic part that reaches every branch, a random part and the refusals; `unit_ssd` is the numpy form of havoc_mi355x_unit_pred_ssd.
"""
import collections
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import sao_decision_tools as T
from sao_merge_tools import bin_cost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# include/havoc_mi355x.h: HAVOC_CU_SYNTAX_CTX_*, HAVOC_CU_CLOSE_*, HAVOC_CU_OUTCOME_*, HAVOC_PU_SYNTAX_CTX_MERGE_IDX
SPLIT_CU_FLAG, CU_SKIP_FLAG, PRED_MODE_FLAG, PART_MODE, RQT_ROOT_CBF, SYNTAX_BYTES = 0, 3, 6, 7, 11, 16
MIN_CB, AMP, MERGE_2Nx2N = 1, 2, 4
REFUSED, CODED, NO_RESIDUAL, SKIPPED = -1, 0, 1, 2
PU_MERGE_IDX = 1
BYPASS = 1 << 16
PART_MODES = ("2Nx2N", "2NxN", "Nx2N", "NxN", "2NxnU", "2NxnD", "nLx2N", "nRx2N")

Slice = collections.namedtuple("Slice", "slice_b max_num_merge_cand reciprocal_lambda")
# the launches of the golden file and of the fresh cases: B and P slices, MaxNumMergeCand 1 and 5, reciprocal lambdas from those of QP 22 to 42
SLICES = [Slice(1, 5, 0.0217), Slice(1, 1, 0.0553), Slice(0, 5, 0.00214), Slice(0, 1, 0.1407)]
REFUSALS = ("flag_bit", "skip_ctx_inc", "log2_cb_size", "log2_3_above_min_cb", "part_mode", "nxn_above_min_cb", "nxn_at_8", "amp_at_min_cb", "amp_disabled",
            "merged_part_mode", "merge_idx", "pu_rate_index", "pu_rate_refused", "tree_rate_refused")


def lambda_q16(d):
    """Lambda::set(double) (turing/FixedPoint.h)"""
    return int(d * 65536 + 0.5)


def i32(v):
    """the int32 an unsigned or wider sum wraps to"""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def tree_of(case, i):
    """what havoc_mi355x_cu_close reads of unit i's decided tree -> (haveResidual, the tree's Q16 rate, int32(ssdY + ssdCb + ssdCr))"""
    ch, tc = case["choice"][i], case["tree_choice"][i]
    zero = int(ch["depth"]) == 0 and int(ch["tried_zero"]) != 0
    mask = int(tc["mask_zero"] if zero else tc["mask_one"])
    ssd_y = int(ch["zero"]["ssd"]) if zero else sum(int(v) for v in ch["one"]["ssd"])
    ssd = i32(ssd_y + int(tc["chroma_ssd_zero"] if zero else tc["chroma_ssd_one"]))
    return mask != 0, int(case["tree_rate"][2 * i + (0 if zero else 1)]), ssd


def refusal(job, M, case):
    """why havoc_mi355x_cu_close does not walk the job (include/havoc_mi355x.h), or None"""
    flags, pm, log2 = int(job["flags"]), int(job["part_mode"]), int(job["log2_cb_size"])
    min_cb = bool(flags & MIN_CB)
    if flags & ~(MIN_CB | AMP | MERGE_2Nx2N):
        return "flag_bit"
    if int(job["skip_ctx_inc"]) > 2:
        return "skip_ctx_inc"
    if not 3 <= log2 <= 6:
        return "log2_cb_size"
    if log2 == 3 and not min_cb:
        return "log2_3_above_min_cb"
    if pm > 7:
        return "part_mode"
    if pm == 3 and not min_cb:
        return "nxn_above_min_cb"
    if pm == 3 and log2 == 3:
        return "nxn_at_8"
    if pm >= 4 and min_cb:
        return "amp_at_min_cb"
    if pm >= 4 and not flags & AMP:
        return "amp_disabled"
    if flags & MERGE_2Nx2N and pm != 0:
        return "merged_part_mode"
    if flags & MERGE_2Nx2N and int(job["merge_idx"]) >= M:
        return "merge_idx"
    if int(job["pu_rate_index"]) < 0:
        return "pu_rate_index"
    if int(case["pu_rate"][int(job["pu_rate_index"])]) < 0:
        return "pu_rate_refused"
    have, rate_tree, _ = tree_of(case, int(job["unit_index"]))
    if have and rate_tree < 0:
        return "tree_rate_refused"
    return None


def close(job, M, lam_q16, case, tags=None):
    """Search<IfCbf<rqt_root_cbf, transform_tree>>::go for one valid job -> (dict of the havoc_mi355x_cu_choice fields, the CU snapshot after, the PU snapshot after)"""
    tags = collections.Counter() if tags is None else tags
    flags, pm, log2, inc = int(job["flags"]), int(job["part_mode"]), int(job["log2_cb_size"]), int(job["skip_ctx_inc"])
    min_cb, amp, merged = bool(flags & MIN_CB), bool(flags & AMP), bool(flags & MERGE_2Nx2N)
    cu0 = [int(v) for v in case["cu_syntax"][int(job["ctx_index"])]]
    pu_before = [int(v) for v in case["pu_before"][int(job["pu_before_index"])]]
    pu_after = [int(v) for v in case["pu_after"][int(job["pu_after_index"])]]
    rate_pu = int(case["pu_rate"][int(job["pu_rate_index"])])
    have, rate_tree, ssd = tree_of(case, int(job["unit_index"]))
    sp = [int(v) for v in case["pred_ssd"][int(job["unit_index"])]]
    dist_coded = lam_q16 * ssd
    ch = case["choice"][int(job["unit_index"])]
    tags["tree", int(ch["depth"]), int(ch["tried_zero"]) != 0, have] += 1
    tags["skip_ctx_inc", inc] += 1

    def decision(syn, ctx, b):
        syn[ctx], r = bin_cost(syn[ctx], int(b))
        return r

    def skipped():
        """the skipped CU from the contexts before the CU: merge_idx when MaxNumMergeCand > 1, cu_skip_flag(1)"""
        cu, pu, rate = list(cu0), list(pu_before), 0
        if M > 1:
            v = int(job["merge_idx"])
            for i in range(v):
                rate += decision(pu, PU_MERGE_IDX, 1) if i == 0 else BYPASS
            if v < M - 1:
                rate += decision(pu, PU_MERGE_IDX, 0) if v == 0 else BYPASS
            tags["skip_merge_idx", M, v] += 1
        else:
            tags["skip_merge_idx_not_coded"] += 1
        rate += decision(cu, CU_SKIP_FLAG + inc, 1)
        return rate, cu, pu

    def preamble():
        """cu_skip_flag(0), pred_mode_flag(0), part_mode (Binarization.h:311-375), after the prediction units"""
        cu, rate = list(cu0), rate_pu
        rate += decision(cu, CU_SKIP_FLAG + inc, 0)
        rate += decision(cu, PRED_MODE_FLAG, 0)
        rate += decision(cu, PART_MODE, pm == 0)
        if pm == 0:
            tags["part_mode", "2Nx2N", "one_bin"] += 1
        else:
            rate += decision(cu, PART_MODE + 1, ~pm >> 1 & 1)
            if min_cb:
                if log2 > 3 and pm != 1:
                    rate += decision(cu, PART_MODE + 2, ~pm >> 2 & 1)
                    tags["part_mode", PART_MODES[pm], "min_cb_third_bin"] += 1
                else:
                    tags["part_mode", PART_MODES[pm], "min_cb_8" if log2 == 3 else "min_cb_two_bins"] += 1
            elif amp:
                rate += decision(cu, PART_MODE + 3, ~pm >> 2 & 1)
                if pm >= 4:
                    rate += BYPASS
                tags["part_mode", PART_MODES[pm], "amp_bypass" if pm >= 4 else "amp_three_bins"] += 1
            else:
                tags["part_mode", PART_MODES[pm], "no_amp_two_bins"] += 1
        return rate, cu

    r = dict(have_residual=int(have), cost_coded=-1)
    if not have and merged:
        tags["skipped_without_residual"] += 1
        r["outcome"] = SKIPPED
        r["rate"], cu, pu = skipped()
        r["lambda_distortion"] = dist_coded
        r["cost_no_residual"] = r["rate"] + dist_coded
    else:
        rate_pre, cu = preamble()
        pu = pu_after
        if not have:
            tags["no_residual_rqt_root_cbf_0"] += 1
            r["outcome"] = NO_RESIDUAL
            r["rate"] = rate_pre + decision(cu, RQT_ROOT_CBF, 0)
            r["lambda_distortion"] = dist_coded
            r["cost_no_residual"] = r["rate"] + dist_coded
        else:
            cu_coded = list(cu)
            rate_coded = rate_pre + rate_tree
            if merged:
                tags["coded_merged_rqt_root_cbf_not_coded"] += 1
            else:
                rate_coded += decision(cu_coded, RQT_ROOT_CBF, 1)
            dist_pred = lam_q16 * sp[0] + lam_q16 * sp[1] + lam_q16 * sp[2]
            if merged:
                rate_none, cu_none, pu_none = skipped()
            else:
                cu_none, pu_none = list(cu), pu_after
                rate_none = rate_pre + decision(cu_none, RQT_ROOT_CBF, 0)
            r["cost_coded"], r["cost_no_residual"] = rate_coded + dist_coded, rate_none + dist_pred
            if r["cost_no_residual"] < r["cost_coded"]:
                tags["skip_wins" if merged else "no_residual_wins"] += 1
                r["outcome"], r["rate"], r["lambda_distortion"], cu, pu = (SKIPPED if merged else NO_RESIDUAL), rate_none, dist_pred, cu_none, pu_none
            else:
                tags["equal_cost_keeps_residual" if r["cost_no_residual"] == r["cost_coded"] else ("coded_wins_merged" if merged else "coded_wins")] += 1
                r["outcome"], r["rate"], r["lambda_distortion"], cu = CODED, rate_coded, dist_coded, cu_coded
    r["cost"] = r["rate"] + r["lambda_distortion"]
    return r, cu, pu


CHOICE_FIELDS = ("outcome", "have_residual", "rate", "lambda_distortion", "cost", "cost_coded", "cost_no_residual")


def refused_record(case, job):
    r = {k: -1 for k in CHOICE_FIELDS}
    r["have_residual"] = 0
    return r, case["cu_syntax"][int(job["ctx_index"])], case["pu_after"][int(job["pu_after_index"])]


def walk_jobs(case, sl, tags=None, closer=None):
    """havoc_mi355x_cu_close over case["jobs"] by the restatement (or by `closer`: Shim.close) -> (CU_CHOICE_DT [n], CU snapshots uint8 [n, 16], PU snapshots
    uint8 [n, 16], refusal reason per job)"""
    from turingcodec_amd.havoc import CU_CHOICE_DT
    tags = collections.Counter() if tags is None else tags
    jobs, M, lam = case["jobs"], sl.max_num_merge_cand, lambda_q16(sl.reciprocal_lambda)
    out, cu_out, pu_out, why = np.zeros(len(jobs), CU_CHOICE_DT), np.zeros((len(jobs), 16), np.uint8), np.zeros((len(jobs), 16), np.uint8), []
    for j, job in enumerate(jobs):
        w = refusal(job, M, case)
        why.append(w)
        if w is not None:
            tags["refused", w] += 1
            r, cu, pu = refused_record(case, job)
        elif closer is not None:
            r, cu, pu = closer(job, sl, case)
        else:
            r, cu, pu = close(job, M, lam, case, tags)
        for k in CHOICE_FIELDS:
            out[k][j] = r[k]
        cu_out[j], pu_out[j] = cu, pu
    return out, cu_out, pu_out, why


def required_tags(sl):
    """the branches the made cases of a launch must reach, by name"""
    M = sl.max_num_merge_cand
    out = ["skipped_without_residual", "no_residual_rqt_root_cbf_0", "coded_merged_rqt_root_cbf_not_coded", "skip_wins", "no_residual_wins", "coded_wins",
           "coded_wins_merged", "equal_cost_keeps_residual", ("part_mode", "2Nx2N", "one_bin")]
    out += [("skip_ctx_inc", i) for i in range(3)]
    out += ["skip_merge_idx_not_coded"] if M == 1 else [("skip_merge_idx", M, i) for i in range(M)]
    out += [("part_mode", PART_MODES[pm], "min_cb_8") for pm in (1, 2)] + [("part_mode", "2NxN", "min_cb_two_bins")]
    out += [("part_mode", PART_MODES[pm], "min_cb_third_bin") for pm in (2, 3)]
    out += [("part_mode", PART_MODES[pm], "amp_three_bins") for pm in (1, 2)] + [("part_mode", PART_MODES[pm], "amp_bypass") for pm in (4, 5, 6, 7)]
    out += [("part_mode", PART_MODES[pm], "no_amp_two_bins") for pm in (1, 2)]
    out += [("tree", 0, True, True), ("tree", 1, True, True), ("tree", 1, False, True), ("tree", 0, False, False), ("tree", 0, True, False), ("tree", 1, True, False)]
    out += [("refused", r) for r in REFUSALS]
    return out


def make_cases(seed, sl, n_random=60, n_states=7):
    """the inputs of one launch -> dict(cu_syntax [k, 16], pu_before [k, 16], pu_after [3 k, 16], pu_rate int64 [n + 1], choice RQT_RESULT_DT [n], tree_choice
    RQT_TREE_RESULT_DT [n], tree_rate int64 [2 n], pred_ssd int32 [n, 3], jobs CU_CLOSE_JOB_DT [n]).  Every part mode at every size with and without MIN_CB / AMP (the
    combinations the writer cannot binarise are the refusals), every context increment, every merge index, trees with and without residual at both depths; the units
    with a residual go round four placements of the prediction's SSD: far above the reconstruction's (coded wins), below it (the unit without residual wins), and --
    with the tree's rate set from the restated preamble -- the two costs EQUAL and one Q16 unit apart either way."""
    from turingcodec_amd.havoc import CU_CLOSE_JOB_DT, RQT_TREE_RESULT_DT
    from turingcodec_amd.decisions import RQT_RESULT_DT
    rng = np.random.default_rng(seed)
    M, lam = sl.max_num_merge_cand, lambda_q16(sl.reciprocal_lambda)
    rows = []

    def job(**kw):
        j = dict(log2_cb_size=int(rng.integers(3, 7)), part_mode=0, skip_ctx_inc=int(rng.integers(0, 3)), merge_idx=int(rng.integers(0, M)), flags=0,
                 residual=bool(rng.integers(0, 2)), depth=int(rng.integers(0, 2)), tried_zero=1, placement=len(rows) % 5, pu_rate=int(rng.integers(0, 60 << 16)),
                 tree_rate=int(rng.integers(1 << 16, 400 << 16)), no_pu_rate=False)
        if j["log2_cb_size"] == 3:
            j["flags"] = MIN_CB
        j.update(kw)
        rows.append(j)

    for log2 in (3, 4, 5, 6):
        for fl in (0, MIN_CB, AMP, MIN_CB | AMP):
            for pm in range(8):
                for residual in (False, True):
                    job(log2_cb_size=log2, flags=fl, part_mode=pm, residual=residual)
    for inc in range(3):
        for residual in (False, True):
            for fl in (0, MERGE_2Nx2N):
                job(skip_ctx_inc=inc, residual=residual, flags=fl | AMP, log2_cb_size=5)
    for idx in range(M):
        for residual in (False, True, True, True, True, True):
            job(flags=MERGE_2Nx2N | (MIN_CB if len(rows) & 1 else 0), merge_idx=idx, residual=residual, log2_cb_size=4 + (len(rows) & 1))
    for depth, tried, residual in ((0, 1, True), (1, 1, True), (1, 0, True), (0, 0, False), (0, 1, False), (1, 1, False)):
        for fl in (0, MERGE_2Nx2N):
            job(depth=depth, tried_zero=tried, residual=residual, flags=fl, log2_cb_size=5)
    for _ in range(n_random):
        lg = int(rng.integers(3, 7))
        fl = (MIN_CB if lg == 3 or rng.random() < 0.3 else 0) | (AMP if rng.random() < 0.5 else 0)
        pm = int(rng.integers(0, 8))
        if rng.random() < 0.35:
            fl, pm = fl | MERGE_2Nx2N, 0
        job(log2_cb_size=lg, flags=fl, part_mode=pm)
    # ---- one job per refusal that the sweep above does not make (include/havoc_mi355x.h)
    job(flags=8)
    job(flags=0x80 | MERGE_2Nx2N)
    job(skip_ctx_inc=3)
    job(skip_ctx_inc=255)
    job(log2_cb_size=2, flags=MIN_CB)
    job(log2_cb_size=7)
    job(part_mode=8, flags=AMP, log2_cb_size=5)
    job(part_mode=255, flags=AMP, log2_cb_size=5)
    job(flags=MERGE_2Nx2N, part_mode=1, log2_cb_size=5)
    job(flags=MERGE_2Nx2N, merge_idx=M, log2_cb_size=5)
    job(flags=MERGE_2Nx2N, merge_idx=255, log2_cb_size=5)
    job(no_pu_rate=True, log2_cb_size=5)
    job(pu_rate=-1, log2_cb_size=5)
    job(tree_rate=-1, residual=True, log2_cb_size=5)
    job(tree_rate=-1, residual=False, log2_cb_size=5, flags=MERGE_2Nx2N)          # not a refusal: without a residual the tree's rate is not read

    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    n = len(rows)
    case = dict(cu_syntax=rng.integers(0, 126, (n_states, 16)).astype(np.uint8), pu_before=rng.integers(0, 126, (n_states, 16)).astype(np.uint8),
                pu_after=rng.integers(0, 126, (3 * n_states, 16)).astype(np.uint8), pu_rate=np.zeros(n + 1, np.int64), choice=np.zeros(n, RQT_RESULT_DT),
                tree_choice=np.zeros(n, RQT_TREE_RESULT_DT), tree_rate=rng.integers(0, 400 << 16, 2 * n).astype(np.int64), pred_ssd=np.zeros((n, 3), np.int32),
                jobs=np.zeros(n, CU_CLOSE_JOB_DT))
    jobs, ch, tc = case["jobs"], case["choice"], case["tree_choice"]
    units, slots = rng.permutation(n), rng.permutation(n)
    for j, row in enumerate(rows):
        for k in ("log2_cb_size", "part_mode", "skip_ctx_inc", "merge_idx", "flags"):
            jobs[k][j] = row[k]
        u = int(units[j])
        jobs["ctx_index"][j], jobs["pu_before_index"][j], jobs["pu_after_index"][j] = rng.integers(0, n_states), rng.integers(0, n_states), rng.integers(0, 3 * n_states)
        jobs["unit_index"][j], jobs["pu_rate_index"][j] = u, -1 if row["no_pu_rate"] else slots[j]
        case["pu_rate"][slots[j]] = row["pu_rate"]
        ch["depth"][u], ch["tried_zero"][u] = row["depth"], row["tried_zero"]
        size = 1 << (2 * row["log2_cb_size"])
        ch["zero"]["ssd"][u] = rng.integers(0, 40 * size)
        ch["one"]["ssd"][u] = rng.integers(0, 10 * size, 4)
        tc["chroma_ssd_zero"][u], tc["chroma_ssd_one"][u] = rng.integers(0, 10 * size, 2)
        # the chosen tree's mask says whether there is a residual; the other depth's is the opposite, so that reading the wrong one shows
        zero = row["depth"] == 0 and row["tried_zero"] != 0
        chosen, other = (int(rng.integers(1, 1 << 20)), 0) if row["residual"] else (0, int(rng.integers(1, 1 << 20)))
        tc["mask_zero"][u], tc["mask_one"][u] = (chosen, other) if zero else (other, chosen)
        case["tree_rate"][2 * u + (0 if zero else 1)] = row["tree_rate"]
        case["pred_ssd"][u] = rng.integers(0, 60 * size, 3)
        if refusal(jobs[j], M, case) is not None or not row["residual"]:
            continue
        # ---- place the two costs (restated rates: what this places is checked on the REFERENCE's results by the golden generator and tests/test_cu_close.py)
        _, _, ssd = tree_of(case, u)
        if row["placement"] == 0:
            case["pred_ssd"][u] = ssd // 3 + row["tree_rate"] // max(lam, 1) + rng.integers(200 * size, 400 * size, 3)
        elif row["placement"] == 1:
            case["pred_ssd"][u] = rng.integers(0, max(ssd // 4, 1), 3)
        else:
            k = int(rng.integers(1, 2000))
            case["pred_ssd"][u] = [ssd, k, 0]
            case["tree_rate"][2 * u + (0 if zero else 1)] = 0
            r, _, _ = close(jobs[j], M, lam, case)
            gap = r["cost_no_residual"] - r["cost_coded"]          # = what the tree's rate must be for equal costs
            while gap + row["placement"] - 3 < 0:
                k += 1 + (-gap) // max(lam, 1)
                case["pred_ssd"][u] = [ssd, k, 0]
                r, _, _ = close(jobs[j], M, lam, case)
                gap = r["cost_no_residual"] - r["cost_coded"]
            case["tree_rate"][2 * u + (0 if zero else 1)] = gap + row["placement"] - 3      # placement 2: coded cheaper by 1; 3: equal; 4: coded dearer by 1
    return case


# ---- the reference's own functions ----------------------------------------------------------------------------------------------------------------
def reference_dir():
    return T.reference_dir()


class Shim:
    """tests/cu_close_shim.cpp over the reference's turing/SyntaxCtu.hpp, Binarization.h, Write.h, CodedData.h and Cabac.cpp, built with oracle/Makefile's TURFLAGS"""

    def __init__(self):
        ref = T.reference_dir()
        assert ref, "reference sources not present"
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libcu_close.so")
        flags = T._make_var("TURFLAGS").split()
        subprocess.check_call(["g++"] + flags + ["-shared", "-o", so, os.path.join(ROOT, "tests", "cu_close_shim.cpp")]
                              + [os.path.join(ref, "turing", f) for f in ("Cabac.cpp", "ScanOrder.cpp")])
        self.L = C.CDLL(so)
        self.L.cu_close_syntax.restype = C.c_int64
        self.L.cu_close_syntax.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        self.L.cu_close_costs.restype = None
        self.L.cu_close_costs.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p]

    def syntax(self, job, sl, skip, cbf, rate_pu, rate_tree, cu, pu):
        """Syntax<coding_unit>::go by the reference -> (rate, CU snapshot, PU snapshot)"""
        flags, log2, inc = int(job["flags"]), int(job["log2_cb_size"]), int(job["skip_ctx_inc"])
        p = np.array([skip, job["part_mode"], log2, log2 if flags & MIN_CB else 3, bool(flags & AMP), inc >= 1, inc >= 2, bool(flags & MERGE_2Nx2N), job["merge_idx"],
                      sl.max_num_merge_cand, cbf, sl.slice_b], np.int32)
        cu, pu = np.array(cu, np.uint8), np.array(pu, np.uint8)
        rate = self.L.cu_close_syntax(p.ctypes.data, int(rate_pu), int(rate_tree), cu.ctypes.data, pu.ctypes.data)
        return int(rate), cu, pu

    def costs(self, rate_coded, ssd, rate_without, ssd_prediction, d):
        """-> (lambdaDistortion coded, cost coded, lambdaDistortion without, cost without, without < coded, Lambda::set(d).value)"""
        out = np.zeros(6, np.int64)
        a, b = np.array(ssd, np.int32), np.array(ssd_prediction, np.int32)
        self.L.cu_close_costs(int(rate_coded), a.ctypes.data, int(rate_without), b.ctypes.data, float(d), out.ctypes.data)
        return [int(v) for v in out]

    def close(self, job, sl, case):
        """the close of one job the contract does not refuse: which syntax is measured from which state is Search.hpp:2412-2531, restated here; every element and
        every cost is the reference's"""
        u, merged = int(job["unit_index"]), bool(int(job["flags"]) & MERGE_2Nx2N)
        cu0 = case["cu_syntax"][int(job["ctx_index"])]
        before, after = case["pu_before"][int(job["pu_before_index"])], case["pu_after"][int(job["pu_after_index"])]
        rate_pu = int(case["pu_rate"][int(job["pu_rate_index"])])
        have, rate_tree, ssd = tree_of(case, u)
        sp = [int(v) for v in case["pred_ssd"][u]]
        r = dict(have_residual=int(have), cost_coded=-1)
        if not have:
            rate, cu, pu = self.syntax(job, sl, int(merged), 0, rate_pu, rate_tree, cu0, before if merged else after)
            dist, cost = self.costs(rate, [ssd, 0, 0], 0, [0, 0, 0], sl.reciprocal_lambda)[:2]
            r.update(outcome=SKIPPED if merged else NO_RESIDUAL, rate=rate, lambda_distortion=dist, cost=cost, cost_no_residual=cost)
            return r, cu, pu
        rate_c, cu_c, pu_c = self.syntax(job, sl, 0, 1, rate_pu, rate_tree, cu0, after)
        rate_n, cu_n, pu_n = self.syntax(job, sl, int(merged), 0, rate_pu, rate_tree, cu0, before if merged else after)
        dist_c, cost_c, dist_n, cost_n, drop, _ = self.costs(rate_c, [ssd, 0, 0], rate_n, sp, sl.reciprocal_lambda)
        r.update(cost_coded=cost_c, cost_no_residual=cost_n)
        if drop:
            r.update(outcome=SKIPPED if merged else NO_RESIDUAL, rate=rate_n, lambda_distortion=dist_n, cost=cost_n)
            return r, cu_n, pu_n
        r.update(outcome=CODED, rate=rate_c, lambda_distortion=dist_c, cost=cost_c)
        return r, cu_c, pu_c


# ---- the decision in numpy and its host form --------------------------------------------------------------------------------------------------------
def decide(have, merged, rate_coded, rate_without, ssd, ssd_prediction, lam_q16):
    """closeInterCu over arrays: have / merged bool [n], the two rates int64 [n], ssd / ssd_prediction int [n, 3] -> int64 [n, 6] = outcome, rate, lambdaDistortion,
    cost, costCoded, costNoResidual"""
    have, merged = np.asarray(have, bool), np.asarray(merged, bool)
    rc, rn = np.asarray(rate_coded, np.int64), np.asarray(rate_without, np.int64)
    s = np.asarray(ssd, np.int64).sum(1).astype(np.uint32).view(np.int32).astype(np.int64)
    dist_c = s * int(lam_q16)
    dist_p = (np.asarray(ssd_prediction, np.int64) * int(lam_q16)).sum(1)
    without = np.where(merged, SKIPPED, NO_RESIDUAL)
    cost_c, cost_n = np.where(have, rc + dist_c, -1), rn + np.where(have, dist_p, dist_c)
    drop = ~have | (cost_n < cost_c)
    rate, dist = np.where(drop, rn, rc), np.where(have & drop, dist_p, dist_c)
    return np.stack([np.where(drop, without, CODED), rate, dist, rate + dist, cost_c, cost_n], 1).astype(np.int64)


class DecisionClient:
    """tests/cu_close_client.cpp: search/cu_decision.hpp's closeInterCu, compiled at test time"""

    def __init__(self):
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libcu_close_client.so")
        subprocess.check_call(["g++", "-O1", "-std=c++14", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "cu_close_client.cpp")])
        self.L = C.CDLL(so)
        self.L.cu_close_decide.restype = C.c_int
        self.L.cu_close_decide.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p]

    def decide(self, have, merged, rate_coded, rate_without, ssd, ssd_prediction, lam_q16):
        n = len(have)
        rows = np.ascontiguousarray(np.concatenate([np.stack([have, merged, rate_coded, rate_without], 1), np.asarray(ssd), np.asarray(ssd_prediction)], 1), np.int64)
        out = np.zeros((n, 6), np.int64)
        assert self.L.cu_close_decide(rows.ctypes.data, n, int(lam_q16), out.ctypes.data) == 0
        return out


# ---- the prediction's distortion ------------------------------------------------------------------------------------------------------------------------
def unit_ssd(src_y, src_stride, src_c, src_stride_c, pred_y, pred_stride, pred_c, pred_stride_c, jobs):
    """havoc_mi355x_unit_pred_ssd in numpy: the flat sample arrays and PRED_SSD_JOB_DT jobs -> int32 [n, 3], each sum wrapped as the reference's int32 accumulator"""
    out = np.zeros((len(jobs), 3), np.int32)
    for i, job in enumerate(jobs):
        for c in range(3):
            n = (1 << int(job["log2_size"])) >> (c > 0)
            a, sa, b, sb = (src_c, src_stride_c, pred_c, pred_stride_c) if c else (src_y, src_stride, pred_y, pred_stride)
            rows = np.arange(n)[:, None]
            cols = np.arange(n)[None, :]
            d = a[int(job["src_off"][c]) + rows * sa + cols].astype(np.int64) - b[int(job["pred_off"][c]) + rows * sb + cols].astype(np.int64)
            out[i, c] = i32(int((d * d).sum()))
    return out
