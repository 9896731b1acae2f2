"""Generators and numpy restatements for tests/test_tu_chain.py: the fused transform-unit chain of csrc/kernels_tu_fused.hip (k_tu_forward and its
SCAN form, k_tu_forward_mfma32, k_tu_reconstruct) held against the oracle at every edge, QP and scan threshold.  Test infrastructure.

Expected values are always the oracle's (`transform`, `quantize_inverse`, `inverse_transform_add`, `ssd`, `rdoq`), composed as suite.LoopImpl.tu_forward /
tu_reconstruct compose them.  The numpy restatements here (the two transforms with their intermediate values, rdoqThresholds, the RdoqInfo record) exist to say
WHICH edge a case reaches -- the four clips of the reconstruction, the three thresholds of the scan -- and are themselves held against the oracle by the CPU tests.
"""
import numpy as np

import cases
import rdoq_tools as rt

ROUTES = [(log2, tr, bd) for (log2, tr) in cases.TRANSFORMS for bd in (8, 9, 10)]


def route_id(route):
    log2, tr, bd = route
    return f"n{1 << log2}{'dst' if tr else 'dct'}-{bd}bit"


def S_of(bd):
    return 1 if bd == 8 else 2


def ragged_counts(log2, mfma=False):
    """1, TPW - 1, TPW, TPW + 1, 2 TPW + 1 with TPW = 64 / N blocks per wavefront (k_tu_forward, k_tu_reconstruct); 1, 2, 9 for the wavefront-per-block MFMA kernel"""
    tpw = 64 >> log2
    c = {1, tpw - 1, tpw, tpw + 1, 2 * tpw + 1}
    if mfma:
        c |= {1, 2, 9}
    return sorted(x for x in c if x > 0)


# ------------------------------------------------------------------------------------------------------------------ the HEVC core transforms in numpy
# Magnitudes of the 32-point matrix by angle (ITU-T H.265 (8-243) .. (8-245)); the smaller DCTs are its even rows.  DST-VII: (8-242).
MAG = [64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4, 0]
DST7 = [[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]]


def basis_matrix(log2, tr):
    """M[k][c], int64"""
    n = 1 << log2
    if tr:
        return np.array(DST7, np.int64)
    m = np.zeros((n, n), np.int64)
    for k in range(n):
        kk = k * (32 // n)
        for c in range(n):
            j = (kk * (2 * c + 1)) & 127
            m[k, c] = 64 if kk == 0 else MAG[j] if j <= 32 else -MAG[64 - j] if j <= 64 else -MAG[j - 64] if j <= 96 else MAG[128 - j]
    return m


def _wrap16(a):
    return ((a + 32768) & 0xffff) - 32768


def np_forward(res, log2, tr, bd):
    """forward transform of residual block(s) [..., n, n] -> (coefficients [..., n, n], largest |first-pass value| before the wrap to 16 bits)"""
    m = basis_matrix(log2, tr)
    s1, s2 = log2 - 1 + bd - 8, log2 + 6
    t_raw = (np.einsum("kj,...ij->...ki", m, np.asarray(res, np.int64)) + (1 << (s1 - 1))) >> s1
    c = (np.einsum("kj,...ij->...ki", m, _wrap16(t_raw)) + (1 << (s2 - 1))) >> s2
    return _wrap16(c), int(np.abs(t_raw).max())


CLIPS = ("dequant", "first_pass", "residual", "sample")


def np_reconstruct(levels, qp, log2, tr, bd, pred):
    """de-quantise -> inverse transform -> add the prediction, one block [n, n]: -> (reconstruction, {(clip, side): reached}) with side -1 = the low bound"""
    m = basis_matrix(log2, tr)
    scale, shift = cases.dequant_params(qp, log2, bd)
    mx = (1 << bd) - 1
    hit = {}

    def clip(name, a, lo, hi):
        hit[(name, -1)] = bool((a < lo).any())
        hit[(name, 1)] = bool((a > hi).any())
        return np.clip(a, lo, hi)

    dq = clip("dequant", (np.asarray(levels, np.int64) * scale + (1 << (shift - 1))) >> shift, -32768, 32767)
    p1 = clip("first_pass", (np.einsum("ik,ij->jk", m, dq) + 64) >> 7, -32768, 32767)
    s2 = 20 - bd
    r = clip("residual", (np.einsum("ik,ij->jk", m, p1) + (1 << (s2 - 1))) >> s2, -32768, 32767)
    rec = clip("sample", np.asarray(pred, np.int64) + r, 0, mx)
    return rec, hit


def clip_is_reachable(clip, log2, tr, bd):
    """whether ANY level block can reach that clip (both sides alike: every stage is odd in its input up to rounding), from the largest value the stage can take:
    |first pass| <= (32768 A + 64) >> 7 and |residual| <= (32768 A + half) >> (20 - bd) with A = the largest column sum of |M|.  The de-quantiser clips once
    32767 * scale >> shift passes 32767 (QP 51 does at every size and bit depth), the sample clip needs a residual of one."""
    a = int(np.abs(basis_matrix(log2, tr)).sum(axis=0).max())
    if clip == "first_pass":
        return (32768 * a + 64) >> 7 > 32767
    if clip == "residual":
        s2 = 20 - bd
        return (32768 * a + (1 << (s2 - 1))) >> s2 > 32767
    return True


# ------------------------------------------------------------------------------------------------------------------ layouts
COEF_SENTINEL = 0x5A5A
LEVEL_SENTINEL = 0x7B7B
SSD_SENTINEL = 0xDEADBEEF


def sample_sentinel(S):
    return 0xA5 if S == 1 else 0xA5A5      # (above every 10-bit sample: it cannot be a reconstruction)


def slot_order(count, seed):
    """a permutation of the slots with job 0 NOT in slot 0 (dead lanes of a ragged wavefront read job 0's parameters)"""
    p = np.random.default_rng(seed).permutation(count)
    if count > 1 and p[0] == 0:
        p[[0, 1]] = p[[1, 0]]
    return p


def strip(blocks, dtype, extra, order=None, fill=0):
    """blocks [count, n, n] side by side in one narrow strip of n rows (tests/test_intra_measure.py's prediction layout): -> (flat array, row stride, offset of block i).
    The stride is n * count + extra: never the plane's."""
    blocks = np.asarray(blocks)
    count, n, _ = blocks.shape
    order = np.arange(count) if order is None else np.asarray(order)
    stride = n * count + extra
    a = np.full((n, stride), fill, dtype)
    for i in range(count):
        a[:, order[i] * n:(order[i] + 1) * n] = blocks[i]
    return a.ravel(), stride, (order * n).astype(np.int32)


def samples_for(res, bd, seed):
    """residual blocks [count, n, n] in [-max, max] -> (source, prediction) sample blocks with source - prediction = residual, at a random common level"""
    res = np.asarray(res, np.int64)
    mx = (1 << bd) - 1
    assert np.abs(res).max() <= mx
    pred = np.where(res >= 0, 0, -res)
    pred = pred + np.random.default_rng(seed).integers(0, mx - np.abs(res) + 1)
    dt = cases.sample_dtype(S_of(bd))
    return (pred + res).astype(dt), pred.astype(dt)


def forward_layout(res, bd, seed):
    """residual blocks -> dict(src, ss, pred, sp, jobs [count, 4], ncoef): source and prediction in strips of different strides, coefficient slots in a shuffled
    order with a sentinel slot before and after"""
    res = np.asarray(res)
    count, n, _ = res.shape
    s, p = samples_for(res, bd, seed)
    o = slot_order(count, seed + 1)
    src, ss, so = strip(s, s.dtype, 4, o)
    pred, sp, po = strip(p, p.dtype, 12, o[::-1])
    co = ((slot_order(count, seed + 2) + 1) * n * n).astype(np.int32)
    jobs = np.stack([co, so, po, np.zeros(count, np.int32)], axis=1).astype(np.int32)
    return dict(src=src, ss=ss, pred=pred, sp=sp, jobs=jobs, ncoef=(count + 2) * n * n)


def oracle_forward(oracle, bd, log2, tr, src, ss, pred, sp, jobs, ncoef):
    """residual (Reconstruct.cpp:258-260) then the forward transform per job, into a sentinel-filled coefficient buffer"""
    n = 1 << log2
    co = np.full(ncoef, COEF_SENTINEL, np.int16)
    res = np.zeros(n * n, np.int16)
    for c, so, po, _ in np.asarray(jobs).tolist():
        oracle.residual(res, 0, n, src, so, ss, pred, po, sp, n, n)
        oracle.transform(co, c, res, 0, n, log2, tr, bd)
    return co


def device_forward(hv, bd, log2, tr, src, ss, pred, sp, jobs, ncoef):
    co = hv.up(np.full(ncoef, COEF_SENTINEL, np.int16))
    hv.tu_forward_d(bd, tr, log2, co, hv.up(src), ss, hv.up(pred), sp, hv.up(np.ascontiguousarray(jobs, np.int32)))
    return hv.down(co, np.int16)


def reconstruct_layout(levels, pred, src, bd, seed, extra_ssd=5):
    """level / prediction / source blocks [count, n, n] -> dict: the three in their own strips, a sentinel-filled reconstruction strip (stride > n), shuffled slots"""
    levels = np.asarray(levels, np.int16)
    count, n, _ = levels.shape
    dt = cases.sample_dtype(S_of(bd))
    S = S_of(bd)
    o = slot_order(count, seed)
    p, sp, po = strip(np.asarray(pred, dt), dt, 12, o)
    s, ss, so = strip(np.asarray(src, dt), dt, 4, o[::-1])
    rec, sr, ro = strip(np.full((count, n, n), sample_sentinel(S), dt), dt, 8, slot_order(count, seed + 1), fill=sample_sentinel(S))
    lo = slot_order(count, seed + 2)
    lv = np.zeros(count * n * n, np.int16)
    for i in range(count):
        lv[lo[i] * n * n:(lo[i] + 1) * n * n] = levels[i].ravel()
    jobs = np.stack([lo * n * n, so, po, ro], axis=1).astype(np.int32)
    return dict(levels=lv, pred=p, sp=sp, src=s, ss=ss, rec=rec, sr=sr, jobs=jobs, nssd=count + extra_ssd)


def oracle_reconstruct(oracle, bd, log2, tr, launches, rec, sr, pred, sp, src, ss, levels, jobs, nssd):
    """havoc_quantize_inverse -> inverse_transform_add -> havoc_ssd(src, rec) per job, in job order, in place on a copy of `rec`; pred None: the prediction is the
    reconstruction buffer itself.  launches: [(qp, first job, end job)].  -> (rec, ssd with SSD_SENTINEL where no job wrote)"""
    n = 1 << log2
    rec = rec.copy()
    ssd = np.full(nssd, SSD_SENTINEL, np.uint32)
    dq = np.zeros(n * n, np.int16)
    jobs = np.asarray(jobs).tolist()
    for qp, lo, hi in launches:
        scale, shift = cases.dequant_params(qp, log2, bd)
        for i in range(lo, hi):
            c, so, po, ro = jobs[i]
            oracle.quantize_inverse(dq, 0, levels, c, scale, shift, n * n)
            oracle.inverse_transform_add(rec, ro, sr, rec if pred is None else pred, po, sp, dq, 0, log2, tr, bd)
            ssd[i] = oracle.ssd(src, so, ss, rec, ro, sr, n, n)
    return rec, ssd


def device_reconstruct(hv, bd, log2, tr, launches, rec, sr, pred, sp, src, ss, levels, jobs, nssd):
    d_rec = hv.up(rec)
    d_pred = d_rec if pred is None else hv.up(pred)
    d_src, d_lv, d_jobs = hv.up(src), hv.up(levels), hv.up(np.ascontiguousarray(jobs, np.int32))
    d_ssd = hv.up(np.full(nssd, SSD_SENTINEL, np.uint32))
    for qp, lo, hi in launches:
        scale, shift = cases.dequant_params(qp, log2, bd)
        hv.tu_reconstruct_d(bd, tr, log2, scale, shift, d_rec, sr, d_pred, sp, d_src, ss, d_lv, d_jobs[lo:hi], d_ssd[lo:])
    return hv.down(d_rec, rec.dtype), hv.down(d_ssd, np.uint32)


# ------------------------------------------------------------------------------------------------------------------ forward cases
def impulse_residuals(n, mx):
    """one block per (y, x) and sign: 0 everywhere but +-max there"""
    out = np.zeros((2 * n * n, n, n), np.int64)
    for i in range(n * n):
        out[2 * i, i // n, i % n] = mx
        out[2 * i + 1, i // n, i % n] = -mx
    return out


def basis_indices(n):
    return list(range(n)) if n <= 8 else [0, 1, 2, n // 2 - 1, n // 2, n - 2, n - 1]


def basis_matched_residuals(log2, tr, mx):
    """residual (y, x) = sign(M[k][y]) sign(M[l][x]) max: the largest magnitude coefficient (k, l) can take.  -> (blocks, [(k, l)])"""
    sg = np.sign(basis_matrix(log2, tr))
    kl = [(k, l) for k in basis_indices(1 << log2) for l in basis_indices(1 << log2)]
    return np.array([np.outer(sg[k], sg[l]) * mx for k, l in kl], np.int64), kl


EXTREME_VALUES = (-129, -128, -1, 0, 127, 128, 255, -255, -256)      # 0x00 / 0x7f / 0x80 / 0xff in the low byte, 0 / -1 in the high byte of the MFMA operand split


def extreme_residuals(n, mx, seed):
    """constants +-max and 0, the two checkerboards, every EXTREME_VALUES constant the bit depth allows, then blocks that mix those values sample by sample"""
    yy, xx = np.mgrid[0:n, 0:n]
    chk = np.where((yy + xx) & 1, -mx, mx)
    vals = [v for v in EXTREME_VALUES if abs(v) <= mx]
    out = [np.full((n, n), mx), np.full((n, n), -mx), np.zeros((n, n), np.int64), chk, -chk] + [np.full((n, n), v) for v in vals]
    rng = np.random.default_rng(seed)
    pool = np.array(vals + [mx, -mx])
    while len(out) < max(2 * (64 // n) + 1, 9) + 6:      # enough blocks for every ragged count
        out.append(rng.choice(pool, (n, n)))
    return np.array(out, np.int64)


# ------------------------------------------------------------------------------------------------------------------ reconstruction cases
CLIP_QPS = (0, 30, 51)


def clip_level_blocks(log2, tr):
    """dense +-32767 and -32768, a lone +-32767 at DC and at (N - 1, N - 1), and the block whose signs follow the basis' first column / row"""
    n = 1 << log2
    rng = np.random.default_rng(40 + log2)
    out = [np.full((n, n), 32767), np.full((n, n), -32767), np.full((n, n), -32768), rng.choice([-32767, 32767], (n, n)), rng.choice([-32768, 32767], (n, n))]
    for y, x in ((0, 0), (n - 1, n - 1)):
        for v in (32767, -32767):
            b = np.zeros((n, n), np.int64)
            b[y, x] = v
            out.append(b)
    sg = np.sign(basis_matrix(log2, tr))
    out += [np.outer(sg[:, 0], sg[:, 0]) * 32767, np.outer(sg[:, 0], sg[:, 0]) * -32767]
    return np.array(out, np.int16)


def clip_cases(log2, tr, bd):
    """-> (levels [count, n, n], pred [count, n, n], launches [(qp, lo, hi)]): every clip_level_blocks block against a prediction of all 0 and of all max, at each CLIP_QPS"""
    lv = clip_level_blocks(log2, tr)
    n = 1 << log2
    mx = (1 << bd) - 1
    levels, pred, launches = [], [], []
    for qp in CLIP_QPS:
        lo = len(levels)
        for p in (0, mx):
            levels += list(lv)
            pred += [np.full((n, n), p)] * len(lv)
        launches.append((qp, lo, len(levels)))
    return np.array(levels, np.int16), np.array(pred), launches


def clip_coverage(log2, tr, bd):
    """{(clip, side)} that clip_cases reaches, from the numpy chain"""
    levels, pred, launches = clip_cases(log2, tr, bd)
    seen = set()
    for qp, lo, hi in launches:
        for i in range(lo, hi):
            _, hit = np_reconstruct(levels[i], qp, log2, tr, bd, pred[i])
            seen |= {k for k, v in hit.items() if v}
    return seen


SPARSE_K = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17)


def sparse_level_blocks(n, seed):
    """only the top-left k x k non-zero (k in SPARSE_K up to n, and n); the same with ONE level just outside the square -- to its right, below it; a lone level
    at the square's outer corner; only row 0; only column 0; the all-zero block"""
    rng = np.random.default_rng(seed)

    def nz(shape):
        return rng.integers(1, 49, shape) * rng.choice([-1, 1], shape)

    out = []
    for k in sorted({k for k in SPARSE_K if k <= n} | {n}):
        b = np.zeros((n, n), np.int64)
        b[:k, :k] = nz((k, k))
        out.append(b)
        if k < n:
            for y, x in ((0, k), (k, 0)):
                c = b.copy()
                c[y, x] = nz(())
                out.append(c)
            c = np.zeros((n, n), np.int64)
            c[k, k] = nz(())
            out.append(c)
    for axis in (0, 1):
        b = np.zeros((n, n), np.int64)
        if axis == 0:
            b[0, :] = nz(n)
        else:
            b[:, 0] = nz(n)
        out.append(b)
    out.append(np.zeros((n, n), np.int64))
    return np.array(out, np.int16)


# ------------------------------------------------------------------------------------------------------------------ the scan folded into the forward transform
# csrc/rdoq_work.h: struct RdoqWork { uint32_t hist[66], cursor[66]; uint32_t otherScans, pad[3]; } rounded up to 16 bytes, then RdoqInfo info[njobs]
# { uint64_t mask, mask2, mask3; int64_t sumSq; }, then uint32_t order[njobs]; havoc_mi355x_rdoq_workspace adds 64 spare bytes
INFO_OFFSET = (2 * 66 * 4 + 4 * 4 + 15) & ~15
INFO_BYTES = 32
INFO_DT = np.dtype([("mask", "<u8"), ("mask2", "<u8"), ("mask3", "<u8"), ("sumSq", "<i8")])
SCAN_QPS = (17, 22, 27, 32, 37, 44)
SCAN_TARGET = 4


def workspace_bytes(njobs):
    return INFO_OFFSET + (INFO_BYTES + 4) * njobs + 64


def rdoq_thresholds(quant_scale, quant_shift):
    """smallest |coefficient| whose rounded level is >= 1, 2, 3 (Rdoq.cpp:108): (|c| scale + half) >> shift >= k  <=>  |c| >= ceil((2 k - 1) half / scale)"""
    half, scale = 1 << (quant_shift - 1), max(int(quant_scale), 1)
    return [-(-(2 * k - 1) * half // scale) for k in (1, 2, 3)]


def group_maxima(coef, n):
    """largest |c| of each 4x4 group of an n x n block: [n / 4, n / 4], (gy, gx)"""
    return np.abs(np.asarray(coef, np.int64).reshape(n // 4, 4, n // 4, 4)).max(axis=(1, 3))


def np_rdoq_info(coef, n, quant_scale, quant_shift):
    """the RdoqInfo record of one block: bit gy * n / 4 + gx of mask / mask2 / mask3 set iff the group's largest |c| >= thr[0] / thr[1] / thr[2]; sumSq = sum c^2"""
    g = group_maxima(coef, n).ravel()
    thr = rdoq_thresholds(quant_scale, quant_shift)
    masks = [sum(1 << i for i in np.flatnonzero(g >= t).tolist()) for t in thr]
    return masks[0], masks[1], masks[2], int((np.asarray(coef, np.int64) ** 2).sum())


def threshold_cells(coef, n, quant_scale, quant_shift):
    """[3, 2]: groups of the block whose largest |c| == thr[m] - 1 / == thr[m]"""
    g = group_maxima(coef, n)
    return np.array([[int((g == t - 1).sum()), int((g == t).sum())] for t in rdoq_thresholds(quant_scale, quant_shift)])


_scan_cache = {}


def scan_case(oracle, bd, log2):
    """The blocks of the scan tests for one (bit depth, size), a fixed seed: the basis-matched DC block, the all-zero residual, 32 blocks of Laplace residuals (scale
    1 .. 48, a small DC offset) whatever they hit, then further such blocks -- kept only when one of their groups lands in a threshold cell that is still short --
    until each of the six cells (m = 0, 1, 2) x (largest |c| of a group == thr[m] - 1, == thr[m]) holds SCAN_TARGET groups.  Everything from the oracle:
    -> dict(res [count, n, n], blocks (rdoq_tools fields), states, coef [count, n * n], levels [count, n * n], cbf [count], info (INFO_DT [count]), cells [3, 2])"""
    key = (bd, log2)
    if key in _scan_cache:
        return _scan_cache[key]
    n = 1 << log2
    mx = (1 << bd) - 1
    rng = np.random.default_rng(9000 + 10 * bd + log2)
    n_states = 7
    states = rng.integers(0, 126, (n_states, 128)).astype(np.uint8)
    res, blocks, coefs = [], [], []
    cells = np.zeros((3, 2), np.int64)

    def draw(r, qp):
        qs, shift, inv = rt.quant_params(qp, log2, bd)
        c = np.zeros(n * n, np.int16)
        oracle.transform(c, 0, np.ascontiguousarray(r, np.int16).ravel(), 0, n, log2, 0, bd)
        k = len(blocks)      # (its index if it is kept): scan 0 mostly, every fifth block scan 1 or 2
        b = dict(log2=log2, c_idx=int(rng.integers(0, 3)) if log2 < 5 else 0, scan_idx=1 + (k // 5) % 2 if k % 5 == 4 else 0, is_intra=int(rng.integers(0, 2)),
                 sdh=int(rng.integers(0, 2)), quant_scale=qs, quant_shift=shift, inv_scale=inv, bit_depth=bd,
                 lam=0.57 * 2 ** ((qp - 12) / 3.0) * float(rng.uniform(0.5, 2)), ctx_index=int(rng.integers(0, n_states)), qp=qp)
        return c, b, threshold_cells(c, n, qs, shift)

    def keep(r, c, b, hit):
        res.append(np.asarray(r, np.int64))
        coefs.append(c)
        blocks.append(b)
        cells[...] += hit

    for r in (np.full((n, n), mx), np.zeros((n, n), np.int64)):
        keep(r, *draw(r, 27))
    draws = 0
    while len(blocks) < 34 or cells.min() < SCAN_TARGET:
        draws += 1
        assert draws < 60000, ("the threshold cells do not fill", bd, log2, cells.tolist())
        r = np.clip(np.rint(rng.laplace(0, float(rng.integers(1, 49)), (n, n))) + int(rng.integers(-3, 4)), -mx, mx)
        c, b, hit = draw(r, int(rng.choice(SCAN_QPS)))
        if len(blocks) < 34 or ((hit > 0) & (cells < SCAN_TARGET)).any():
            keep(r, c, b, hit)
    count = len(blocks)
    levels = np.zeros((count, n * n), np.int16)
    cbf = np.zeros(count, np.int32)
    info = np.zeros(count, INFO_DT)
    for i, b in enumerate(blocks):
        levels[i], cbf[i] = oracle.rdoq(np.ascontiguousarray(coefs[i]), log2, b["c_idx"], b["scan_idx"], b["is_intra"], b["sdh"], b["quant_scale"], b["quant_shift"],
                                        b["inv_scale"], bd, b["lam"], np.ascontiguousarray(states[b["ctx_index"]]))
        info[i] = np_rdoq_info(coefs[i], n, b["quant_scale"], b["quant_shift"])
    out = dict(res=np.array(res), blocks=blocks, states=states, coef=np.array(coefs), levels=levels, cbf=cbf, info=info, cells=cells)
    _scan_cache[key] = out
    return out


def scan_layout(case, bd, log2, seed=77):
    """source / prediction strips and the two job tables of a scan launch: the rdoq job's src_off = the TU job's coef_off, its dst_off another slot order, not job order"""
    from turingcodec_amd import havoc
    n2 = 1 << 2 * log2
    lay = forward_layout(case["res"], bd, seed)
    count = len(case["blocks"])
    dst = (((lay["jobs"][:, 0] // n2 - 1 + count // 2 + 1) % count + 1) * n2).astype(np.int32)      # the coefficient slot rotated by half the table: never the same offset
    blocks = [dict(b, src_off=int(lay["jobs"][i, 0])) for i, b in enumerate(case["blocks"])]
    rj = rt.device_jobs(blocks, havoc.rdoq_lambda)
    rj["dst_off"] = dst
    lay.update(rjobs=rj, nlevel=(count + 2) * n2)
    return lay


def expected_buffers(case, lay, log2, count):
    """what the first `count` jobs leave in sentinel-filled buffers: (coefficients, zeroed level buffer, final level buffer)"""
    n2 = 1 << 2 * log2
    co = np.full(lay["ncoef"], COEF_SENTINEL, np.int16)
    zero = np.full(lay["nlevel"], LEVEL_SENTINEL, np.int16)
    lv = zero.copy()
    for i in range(count):
        c, d = int(lay["jobs"][i, 0]), int(lay["rjobs"]["dst_off"][i])
        co[c:c + n2] = case["coef"][i]
        zero[d:d + n2] = 0
        lv[d:d + n2] = case["levels"][i]
    return co, zero, lv
