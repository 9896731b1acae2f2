"""The rate the reference's EstimateRate verb measures for one residual_coding (turing/EncodeResidual.hpp:36-301 over what CodedData::storeResidual,
turing/CodedData.h:457-517, packs from a raster of levels), restated on the CPU in plain Python.  Test infrastructure.

Rates are integers (Cost = FixedPoint<int64_t, 16>): a context-coded bin costs measureEncodeDecision (sao_merge_tools.bin_cost: the tables of
turingcodec_amd/csrc/cabac_tables.h, which the device uses too) and moves its context, a bypass bin 1 << 16.  `walk_block` follows the reference's two steps -- pack
the sub-blocks' flag words and remaining levels, then walk them -- and counts the branches it takes in `tags` (a collections.Counter), in the manner of
deblock_tools.py.  `Shim` compiles tests/residual_rate_shim.cpp -- the reference's own storeResidual and EncodeResidual::inner over a stand-in handle -- into a
temporary directory.  `make_cases` makes the blocks: most are the levels the oracle's RDOQ makes from rdoq_tools.make_blocks, the rest are hand-made for the rare
branches; chains of 1..4 blocks share a job.
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

# the flat 128-byte snapshot (include/havoc_mi355x.h: HAVOC_RDOQ_CTX_*)
LAST_X, LAST_Y, CSBF, SIG, GREATER1, GREATER2 = 8, 26, 44, 48, 92, 116
RESIDUAL_BYTES = np.r_[8:122]          # the contexts residual_coding touches

GROUP_IDX = [0, 1, 2, 3, 4, 4, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7] + [8] * 8 + [9] * 8      # Write.h:1284
SIG_MAP_4X4 = [0, 1, 4, 5, 2, 3, 4, 5, 6, 6, 8, 8, 7, 7, 8, 8]                        # Write.h:1303-1309
SIG_MAP = [[2, 1, 1, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0], [2, 2, 2, 2, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0],
           [2, 1, 0, 0, 2, 1, 0, 0, 2, 1, 0, 0, 2, 1, 0, 0], [2] * 16]               # Write.h:1331-1355


def scan_xy(size, scan_idx):
    """ScanOrder.h:31-97: [(x, y)] of a size x size block in scan order"""
    if scan_idx == 1:
        return [(i % size, i // size) for i in range(size * size)]
    if scan_idx == 2:
        return [(i // size, i % size) for i in range(size * size)]
    out = []
    for d in range(2 * size - 1):
        for x in range(d + 1):
            if x < size and d - x < size:
                out.append((x, d - x))
    return out


_SCANS = {(s, k): scan_xy(s, k) for s in (1, 2, 4, 8) for k in (0, 1, 2)}


def walk_block(block, log2, c_idx, scan_idx, sdh, st, tags=None, touched=None):
    """block: int [n, n] levels; st: list of 128 context states, updated in place -> the Q16 rate.  touched: the set of contexts the chain has moved so far."""
    tags = collections.Counter() if tags is None else tags
    touched = set() if touched is None else touched
    n, gw = 1 << log2, 1 << (log2 - 2)
    raster_s, raster_c = _SCANS[gw, scan_idx], _SCANS[4, scan_idx]
    rate = 0
    reads_moved = [False]

    def decision(ctx, b):
        nonlocal rate
        if ctx in touched:
            reads_moved[0] = True
        st[ctx], r = bin_cost(st[ctx], b)
        rate += r
        moved.add(ctx)

    moved = set()
    # ---- CodedData::storeResidual: per sub-block in scan order the flag words (bit 15 - n = scan position n) and the levels > 1
    subs = []
    for i in range(gw * gw):
        xs, ys = raster_s[i]
        sig = g1 = 0
        rem = []
        for pos in range(15, -1, -1):
            x, y = raster_c[pos]
            v = int(block[4 * ys + y, 4 * xs + x])
            if v != 0:
                sig |= 1 << (15 - pos)
                if v < 0:
                    v = ((-v + 32768) & 0xFFFF) - 32768      # `value = -value` in int16: -32768 stays
                if v > 1:
                    g1 |= 1 << (15 - pos)
                    rem.append(v & 0xFFFF)
        subs.append((sig, g1, rem))
    coded = [s[0] != 0 for s in subs]
    if not any(coded):
        tags["zero_block"] += 1
        return 0
    tags["scan", scan_idx] += 1
    tags["c_idx", c_idx] += 1
    last_sub = max(i for i in range(gw * gw) if coded[i])
    sig_last = subs[last_sub][0]
    last_pos = 15 - ((sig_last & -sig_last).bit_length() - 1)
    if sum(bin(s[0]).count("1") for s in subs) == 1:
        tags["dc_only" if last_sub == 0 and last_pos == 0 else "lone"] += 1
        if last_sub == gw * gw - 1 and last_pos == 15:
            tags["lone_last"] += 1
    # ---- the last position (EncodeResidual.hpp:60-81, Binarization.h:854-931)
    xc, yc = 4 * raster_s[last_sub][0] + raster_c[last_pos][0], 4 * raster_s[last_sub][1] + raster_c[last_pos][1]
    if scan_idx == 2:
        xc, yc = yc, xc
        tags["swap"] += 1
    cmax = 2 * log2 - 1
    off, shift = (15, log2 - 2) if c_idx else (3 * (log2 - 2) + ((log2 - 1) >> 2), (log2 + 1) >> 2)
    for base, v, name in ((LAST_X, xc, "x"), (LAST_Y, yc, "y")):
        prefix = GROUP_IDX[v]
        for b in range(min(prefix, cmax)):
            decision(base + off + (b >> shift), 1)
        if prefix < cmax:
            decision(base + off + (prefix >> shift), 0)
        else:
            tags["last_prefix_max", name] += 1
        if prefix > 3:
            rate += ((prefix >> 1) - 1) << 16
            tags["last_gt3", name] += 1
    last_g1, g1ctx, snake = 1, -1, 0
    for i in range(last_sub, -1, -1):
        xs, ys = raster_s[i]
        sig_actual, g1_flags, rem = subs[i] if coded[i] else (0, 0, [])
        d = 7 + ys - xs
        nb = (snake >> d) & 3
        snake &= ~(3 << d)
        if coded[i]:
            snake |= 3 << d
        infer = 0
        if i != last_sub and i != 0:
            decision(CSBF + (2 if c_idx else 0) + (1 if nb else 0), int(coded[i]))
            tags["csbf", int(coded[i]), nb] += 1
            infer = 1
        if not (coded[i] or i == 0):
            continue
        if not coded[i]:
            tags["empty_sb0"] += 1
        # sig_coeff_flag (:113-135, Write.h:1292-1392)
        sig = sig_actual
        if sig & 0x7FFF:
            infer = 0
        if infer:
            tags["infer_dc"] += 1
        mask = 0x7FFF if infer else 0xFFFF
        pos = 15
        if i == last_sub:
            mask >>= 16 - last_pos
            sig >>= 16 - last_pos
            pos = last_pos - 1
        while mask:
            x, y = raster_c[pos]
            rp = 4 * y + x
            if log2 == 2:
                inc = SIG_MAP_4X4[rp]
            elif i == 0 and rp == 0:
                inc = 0
            else:
                inc = SIG_MAP[nb][rp]
                if c_idx == 0:
                    inc += (3 if i != 0 else 0) + ((9 if scan_idx == 0 else 15) if log2 == 3 else 21)
                else:
                    inc += 9 if log2 == 3 else 12
            decision(SIG + (27 if c_idx else 0) + inc, sig & 1)
            sig >>= 1
            mask >>= 1
            pos -= 1
        # coeff_abs_level_greater1_flag, with greater2 inside the loop (:137-183)
        ctx_set = (2 if (i != 0 and c_idx == 0) else 0) | (1 if ((g1ctx > 0 and last_g1) or g1ctx == 0) else 0)
        if coded[i] and ctx_set & 1:
            tags["ctxset_odd"] += 1
        g1ctx = 1
        base = GREATER1 + ctx_set * 4 + (16 if c_idx else 0)
        num, greater2, k = 0, -1, 0
        flags, g1f = sig_actual, g1_flags
        while flags:
            if flags & 1:
                f = g1f & 1
                decision(base + g1ctx, f)
                if g1ctx > 0:
                    last_g1 = f
                if f and greater2 < 0:
                    greater2 = 1 if rem[k] > 2 else 0
                    decision(GREATER2 + ctx_set + (4 if c_idx else 0), greater2)
                    tags["g2", greater2] += 1
                num += 1
                if num == 8:
                    if flags >> 1:
                        tags["more_than_8"] += 1
                    break
                k += f
                if last_g1:
                    g1ctx = 0
                elif g1ctx < 3:
                    g1ctx += 1
            g1f >>= 1
            flags >>= 1
        # coeff_sign_flag (:189-249)
        bits = bin(sig_actual).count("1")
        if sdh and (sig_actual & 0x1FFF):
            first = min(p for p in range(16) if sig_actual & (1 << (15 - p)))
            last = max(p for p in range(16) if sig_actual & (1 << (15 - p)))
            hidden = int(last - first > 3)
            tags["sign_hidden", hidden] += 1
            bits -= hidden
        elif coded[i] and not sdh:
            tags["sdh0"] += 1
        rate += bits << 16
        # coeff_abs_level_remaining (:262-289, Binarization.h:1199-1238)
        rice, cd1, cd2, k = 0, 0b100111, 0b011110, 0
        flags, g1f = sig_actual, g1_flags
        while flags:
            if flags & 1:
                g = g1f & 1
                a = rem[k] if g else 1
                if a == 32767:
                    tags["mag32767"] += 1
                b = cd1 >> 4
                b += (b + cd2) >> 5
                cd1 -= 1
                cd2 -= g
                k += g
                r = a - b
                if r >= 0:
                    nb_ = rice + 4
                    e = (r >> rice) - 3
                    if e < 0:
                        nb_ += e
                    else:
                        nb_ += 2 * ((e + 1).bit_length() - 1)
                        tags["escape"] += 1
                    rice = min(rice + (1 if a > 3 * (1 << rice) else 0), 4)
                    if rice == 4:
                        tags["rice4"] += 1
                    rate += nb_ << 16
            g1f >>= 1
            flags >>= 1
    if reads_moved[0]:
        tags["reads_moved"] += 1
    touched |= moved
    return rate


def walk_jobs(log2, levels, states, jobs, tags=None):
    """the device's contract: -> (int64 rates [max rate_index + count] (entries no job writes 0), uint8 states after [njobs, 128])"""
    tags = collections.Counter() if tags is None else tags
    n2 = 1 << 2 * log2
    n = 1 << log2
    nr = int((jobs["rate_index"].astype(np.int64) + np.clip(jobs["count"], 1, 4)).max()) if len(jobs) else 0
    rates = np.zeros(nr, np.int64)
    after = np.zeros((len(jobs), 128), np.uint8)
    for j, job in enumerate(jobs):
        st = [int(v) for v in states[int(job["ctx_index"])]]
        count, c_idx, scan = int(job["count"]), int(job["c_idx"]), int(job["scan_idx"])
        if not (1 <= count <= 4 and c_idx <= 2 and scan <= 2 and (scan == 0 or log2 <= 3) and (c_idx == 0 or log2 <= 4)):
            rates[int(job["rate_index"]):int(job["rate_index"]) + min(max(count, 1), 4)] = -1
            after[j] = st
            continue
        touched = set()
        for k in range(count):
            o = int(job["level_off"]) + k * n2
            before = tags["reads_moved"]
            rates[int(job["rate_index"]) + k] = walk_block(levels[o:o + n2].reshape(n, n), log2, c_idx, scan, int(job["sdh"]), st, tags, touched)
            if k and tags["reads_moved"] > before:
                tags["chain", count] += 1
        after[j] = st
    return rates, after


# ---- blocks ---------------------------------------------------------------------------------------------------------------------------------
def special_blocks(rng, log2):
    """hand-made blocks for the rare branches: [(int16 [n, n], c_idx, scan_idx, sdh)]"""
    n, gw = 1 << log2, 1 << (log2 - 2)
    out = []

    def blank():
        return np.zeros((n, n), np.int16)

    comps = (0, 1, 2) if log2 <= 4 else (0,)
    scans = (0, 1, 2) if log2 <= 3 else (0,)
    out.append((blank(), 0, 0, 1))
    for c in comps:
        for s in scans:
            b = blank()
            b[0, 0] = -3
            out.append((b, c, s, 1))
            b = blank()
            b[n - 1, n - 1] = 1                      # a lone coefficient at the last scan position: maximum prefixes, suffix bins
            out.append((b, c, s, int(rng.integers(0, 2))))
            b = blank()
            b[min(1, n - 1), n - 2] = -2             # x > y: scan_idx 2 swaps them
            out.append((b, c, s, 1))
    # a large level at every position in turn would be long: dense sub-blocks with large, growing magnitudes (the Rice parameter reaches 4, escape codes)
    for k in range(3):
        b = blank()
        b[:4, :4] = rng.choice([-1, 1], (4, 4)) * rng.integers(1, [4, 40, 3000][k], (4, 4))
        b[0, 0] = 32767
        b[3, 3] = [-32767, 32767, -32768][k]
        if gw > 1:
            b[4:8, 4:8] = rng.integers(-2, 3, (4, 4))
        out.append((b.astype(np.int16), 0, 0, k & 1))
    # sub-block patterns: empty / DC only / sparse / dense, so that every neighbour pattern of an uncoded and of a coded sub-block occurs, the DC flag is
    # inferred, sub-block 0 is empty below a coded one, and the greater1 context set carries over
    if gw > 1:
        for k in range(24 if log2 < 5 else 12):
            b = blank()
            p = float(rng.choice([0.25, 0.5, 0.8]))
            for ys in range(gw):
                for xs in range(gw):
                    kind = rng.random()
                    if rng.random() > p or (k % 3 == 0 and xs + ys == 0):
                        continue
                    sb = b[4 * ys:4 * ys + 4, 4 * xs:4 * xs + 4]
                    if kind < 0.3:
                        sb[0, 0] = int(rng.choice([-2, -1, 1, 3]))
                    elif kind < 0.6:
                        sb[int(rng.integers(0, 4)), int(rng.integers(0, 4))] = int(rng.choice([-1, 1, 2, -5]))
                    elif kind < 0.8:
                        sb[...] = rng.choice([-1, 1], (4, 4)) * (rng.random((4, 4)) < 0.7)
                    else:
                        sb[...] = rng.integers(-3, 4, (4, 4))
            out.append((b, int(rng.choice(comps)), int(rng.choice(scans)), int(rng.integers(0, 3) > 0)))
    else:
        for k in range(12):
            b = (rng.integers(-3, 4, (4, 4)) * (rng.random((4, 4)) < [0.3, 0.6, 1.0][k % 3])).astype(np.int16)
            out.append((b, int(rng.choice(comps)), int(rng.choice(scans)), int(rng.integers(0, 3) > 0)))
    return out


def make_cases(oracle, seed, log2, rdoq_count, n_states=7, bd=8):
    """-> (levels int16 [blocks * n * n], states uint8 [n_states, 128], jobs RESIDUAL_RATE_JOB_DT): rdoq_count blocks quantised by the oracle's RDOQ from
    rdoq_tools.make_blocks plus special_blocks, shuffled into jobs that chain 1..4 blocks of one component and scan"""
    import rdoq_tools as rt
    from turingcodec_amd.havoc import RESIDUAL_RATE_JOB_DT
    rng = np.random.default_rng(seed)
    n2 = 1 << 2 * log2
    src, states, blocks = rt.make_blocks(seed, log2, bd, rdoq_count, n_states=n_states)
    lv, _ = rt.run_cpu(oracle, src, states, blocks)
    # (make_blocks scans some larger blocks horizontally / vertically for the quantiser's sake; the encoder does so up to 8x8 only: the diagonal scan here)
    items = [(lv[b["src_off"]:b["src_off"] + n2], b["c_idx"], b["scan_idx"] if log2 <= 3 else 0, b["sdh"]) for b in blocks]
    items += [(b.ravel(), c, s, sdh) for b, c, s, sdh in special_blocks(rng, log2)]
    order = rng.permutation(len(items))
    levels, jobs, k = [], [], 0
    while k < len(order):
        count = int(rng.choice([1, 1, 2, 3, 4]))
        chain = [items[i] for i in order[k:k + count]]
        k += count
        _, c, s, sdh = chain[0]
        jobs.append((len(levels) * n2, int(rng.integers(0, n_states)), len(levels), c, s, sdh, len(chain), (0, 0, 0, 0)))
        levels += [it[0] for it in chain]
    return np.concatenate(levels).astype(np.int16), states, np.array(jobs, RESIDUAL_RATE_JOB_DT)


# what the blocks used on the device must reach, per transform size (a 4x4 block has one sub-block: no flag of one, and the odd context sets need a sub-block
# visited before; an 8x8 block's middle sub-blocks 1 and 2 always have
# sub-block 3 -- coded, being the last -- to their right or below unless the last is sub-block 2, so their pattern is never 3 and a coded one's never 0)
def required_tags(log2):
    req = ["zero_block", "dc_only", "lone_last", "more_than_8", ("g2", 0), ("g2", 1), ("sign_hidden", 0), ("sign_hidden", 1), "sdh0", "rice4", "escape",
           "mag32767", ("chain", 2), ("chain", 3), ("chain", 4), ("scan", 0), ("c_idx", 0)]
    if log2 <= 3:
        req += [("scan", 1), ("scan", 2), "swap"]
    if log2 <= 4:
        req += [("c_idx", 1), ("c_idx", 2)]
    if log2 >= 3:
        req += ["ctxset_odd", ("last_gt3", "x"), ("last_gt3", "y"), ("last_prefix_max", "x"), ("last_prefix_max", "y"), "infer_dc", "empty_sb0"]
        req += [("csbf", 0, nb) for nb in ((0, 1, 2) if log2 == 3 else (0, 1, 2, 3))]
        req += [("csbf", 1, nb) for nb in ((1, 2) if log2 == 3 else (0, 1, 2, 3))]
    return req


# ---- the reference's own functions ----------------------------------------------------------------------------------------------------------------
def reference_dir():
    return T.reference_dir()


class Shim:
    """tests/residual_rate_shim.cpp over the reference's turing/EncodeResidual.hpp, CodedData.h, Cabac.cpp and ScanOrder.cpp, built with oracle/Makefile's TURFLAGS"""

    def __init__(self):
        ref = T.reference_dir()
        assert ref, "reference sources not present"
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libresidual_rate.so")
        flags = T._make_var("TURFLAGS").split()
        subprocess.check_call(["g++"] + flags + ["-shared", "-o", so, os.path.join(ROOT, "tests", "residual_rate_shim.cpp")]
                              + [os.path.join(ref, "turing", f) for f in ("Cabac.cpp", "ScanOrder.cpp")])
        self.L = C.CDLL(so)
        self.L.residual_rate_chain.restype = None
        self.L.residual_rate_chain.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]

    def walk_jobs(self, log2, levels, states, jobs):
        """walk_jobs by the reference (valid jobs only)"""
        n2 = 1 << 2 * log2
        levels = np.ascontiguousarray(levels, np.int16)
        nr = int((jobs["rate_index"].astype(np.int64) + jobs["count"]).max()) if len(jobs) else 0
        rates = np.zeros(nr, np.int64)
        after = np.zeros((len(jobs), 128), np.uint8)
        for j, job in enumerate(jobs):
            st = np.ascontiguousarray(states[int(job["ctx_index"])], np.uint8).copy()
            r = np.zeros(4, np.int64)
            o = int(job["level_off"])
            blk = np.ascontiguousarray(levels[o:o + int(job["count"]) * n2])
            self.L.residual_rate_chain(blk.ctypes.data, int(job["count"]), log2, int(job["c_idx"]), int(job["scan_idx"]), int(job["sdh"]), st.ctypes.data, r.ctypes.data)
            rates[int(job["rate_index"]):int(job["rate_index"]) + int(job["count"])] = r[:int(job["count"])]
            after[j] = st
        return rates, after


# ---- search/tu_decision.hpp: decideRqt with a rate per candidate, in numpy -----------------------------------------------------------------------------
def tu_rate(cbf, nonzero, sum_abs):
    """the stand-in: (1 + (cbf ? 2 nonzero + sum_abs : 0)) << 16"""
    return (1 + np.where(np.asarray(cbf) != 0, 2 * np.asarray(nonzero, np.int64) + np.asarray(sum_abs, np.int64), 0)).astype(np.int64) << 16


def decide_rqt(units, zero_at, one_at, sizes, rl_q16):
    """units: RQT_CU_DT; sizes: {log2: dict(cbf, ssd, rate[, nonzero, sum_abs]) per candidate} -> RQT_RESULT_DT records as havoc_mi355x_rqt_decide(_rated) writes them:
    depth 1 first; none of its blocks coded -> depth 1 stands and depth 0 is never looked at; else depth 0 wins on cost_zero < cost_one"""
    from turingcodec_amd.decisions import RQT_RESULT_DT
    out = np.zeros(len(units), RQT_RESULT_DT).view(np.int32).reshape(len(units), 26)
    cost = np.zeros((len(units), 2), np.int64)
    for i, u in enumerate(units):
        L = int(u["log2_size"])
        s0, s1, j0, j1 = sizes[L], sizes[L - 1], int(zero_at[i]), int(one_at[i])

        def outcome(s, j):
            return [int(s["cbf"][j]), int(np.array(s["ssd"][j], np.uint32).view(np.int32)),      # (the SSD enters the cost as int32, as in the reference)
                    int(s["nonzero"][j]) if "nonzero" in s else 0, int(s["sum_abs"][j]) if "sum_abs" in s else 0]

        ssd_one = rate_one = 0
        coded = False
        for k in range(4):
            out[i, 6 + 4 * k:10 + 4 * k] = outcome(s1, j1 + k)
            ssd_one += int(out[i, 7 + 4 * k])
            coded |= s1["cbf"][j1 + k] != 0
            rate_one += int(s1["rate"][j1 + k])
        cost[i, 1] = rate_one + rl_q16 * ssd_one
        depth = tried = 0
        if coded:
            tried = 1
            out[i, 2:6] = outcome(s0, j0)
            cost[i, 0] = int(s0["rate"][j0]) + rl_q16 * int(out[i, 3])
            depth = 0 if cost[i, 0] < cost[i, 1] else 1
        out[i, 0], out[i, 1] = depth, tried
    rec = out.reshape(-1).view(RQT_RESULT_DT).copy()
    rec["cost_zero"], rec["cost_one"] = cost[:, 0], cost[:, 1]
    return rec
