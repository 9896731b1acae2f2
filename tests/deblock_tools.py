"""The in-loop deblocking of a picture (LoopFilter::Picture::deblock<EDGE_VER> then <EDGE_HOR> with LumaBlockEdge / ChromaBlockEdge,
turing/LoopFilter.h:229-400, 739-777) restated with numpy, and seeded pictures for it.  Test infrastructure.

`make_picture` draws every parameter independently of the content: QpY 0..51 per 8x8 region, the disabled bit, strengths 0 / 1 / 2, both
slice offsets over -6..6 (a share of the pictures with beta >= 3 and tc <= -3: what reaches the strong filter's clip), the two chroma QP
offsets over -12..12; content that is blocky and smooth at a dark, a middle or a bright level, so that Clip1 is reached at both ends.

`restate` is vectorised over the edge segments of one direction (one boolean mask per branch), horizontal edges being the vertical edges of
the transposed planes and block map.  `tags` (a collections.Counter) receives, per edge direction (V / H), the number of segments that took
each branch and histograms of the table indices: names in `luma_tags()` / `chroma_tags()`, `<dir>.luma.beta_idx.<i>`, `<dir>.luma.tc_idx.<i>`
(segments past the dE test), `<dir>.luma.tc_clip_idx.<i>` (segments in which tC limited an output: the entries a wrong constant would show
in), `<dir>.<cb|cr>.tc_idx.<i>`.
"""
import collections

import numpy as np

BETA = np.array([0] * 16 + list(range(6, 19)) + list(range(20, 66, 2)), np.int64)                            # H.265 table 8-12, Q = 0..51
TC = np.array([0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24], np.int64)   # Q = 0..53
QPC_30_42 = np.array([29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37], np.int64)                         # H.265 table 8-10 (4:2:0), qPi = 30..42
assert len(BETA) == 52 and len(TC) == 54

ENABLES = ("PQ", "Pq", "pQ", "pq")      # upper case: that side's region has the filter enabled
DIRS = ("V", "H")


def luma_tags():
    t = ["bS1", "bS2", "beta_exit", "strong_clipped", "line_skipped_10tc", "line_skipped_big_tc", "delta_clipped", "p1_clipped", "q1_clipped", "clip_lo",
         "clip_hi", "tc0"]
    t += ["strong_" + e for e in ENABLES]
    t += [f"normal_{e}_dEp{a}_dEq{b}" for e in ENABLES for a in (0, 1) for b in (0, 1)]
    return [f"{d}.luma.{k}" for d in DIRS for k in t]


def chroma_tags():
    t = list(ENABLES) + ["delta_clipped", "clip_lo", "clip_hi", "qpi_neg", "qpi_0_29", "qpi_30_42", "qpi_gt42", "bs1_ignored"]
    return [f"{d}.{p}.{k}" for d in DIRS for p in ("cb", "cr") for k in t]


def chroma_tc_indices():
    """every tc index a chroma segment can read with QpY 0..51, a QP offset of -12..12 and tc_offset_div2 of -6..6"""
    out = set()
    for qpl in range(52):
        for off in range(-12, 13):
            qpi = qpl + off
            qpc = qpi if qpi < 30 else (qpi - 6 if qpi > 42 else int(QPC_30_42[qpi - 30]))
            for tc2 in range(-6, 7):
                out.add(min(53, max(0, qpc + 2 + 2 * tc2)))
    return out


def _en(on_p, on_q):
    """the four enable combinations as (name, mask)"""
    return (("PQ", on_p & on_q), ("Pq", on_p & ~on_q), ("pQ", ~on_p & on_q), ("pq", ~on_p & ~on_q))


def _luma_pass(P, bs2, qp, on, tc2, beta2, bd, tags, name):
    """the luma edges ACROSS the second axis of P (P = the plane for vertical edges, its transpose for horizontal ones), in place.
    bs2[pos], qp, on: [region along the edge, region across it]"""
    n_al, n_ac = P.shape[0] // 8, P.shape[1] // 8
    assert not bs2[0][:n_al, 0].any() and not bs2[1][:n_al, 0].any(), "a strength on the picture boundary: block P does not exist"
    if n_ac < 2:
        return
    mx, sc = (1 << bd) - 1, 1 << (bd - 8)
    v = np.array(P[:, 4:-4]).reshape(n_al, 2, 4, n_ac - 1, 8)        # [region, position, line, edge, p3 p2 p1 p0 q0 q1 q2 q3]
    p3, p2, p1, p0, q0, q1, q2, q3 = (v[..., j] for j in range(8))
    seg = lambda a: a[:, None, None, :]
    bS = np.stack([bs2[0][:n_al, 1:n_ac], bs2[1][:n_al, 1:n_ac]], 1)[:, :, None, :]
    qpP, qpQ = seg(qp[:n_al, 0:n_ac - 1]), seg(qp[:n_al, 1:n_ac])
    onP, onQ = seg(on[:n_al, 0:n_ac - 1]), seg(on[:n_al, 1:n_ac])
    onP, onQ = np.broadcast_to(onP, bS.shape), np.broadcast_to(onQ, bS.shape)
    qPL = (qpQ + qpP + 1) >> 1
    bidx = np.clip(qPL + (beta2 << 1), 0, 51) + 0 * bS
    tidx = np.clip(qPL + 2 * (bS - 1) + (tc2 << 1), 0, 53)
    beta, tC = BETA[bidx] * sc, TC[tidx] * sc
    L = lambda a, k: a[:, :, k:k + 1, :]
    dp0, dp3 = abs(L(p2, 0) - 2 * L(p1, 0) + L(p0, 0)), abs(L(p2, 3) - 2 * L(p1, 3) + L(p0, 3))
    dq0, dq3 = abs(L(q2, 0) - 2 * L(q1, 0) + L(q0, 0)), abs(L(q2, 3) - 2 * L(q1, 3) + L(q0, 3))
    active = bS > 0
    passed = active & (dp0 + dq0 + dp3 + dq3 < beta)

    def dsam(k, dpq):
        return (2 * dpq < (beta >> 2)) & (abs(L(p3, k) - L(p0, k)) + abs(L(q0, k) - L(q3, k)) < (beta >> 3)) & (abs(L(p0, k) - L(q0, k)) < ((5 * tC + 1) >> 1))
    strong = passed & dsam(0, dp0 + dq0) & dsam(3, dp3 + dq3)
    normal = passed & ~strong
    side = (beta + (beta >> 1)) >> 3
    dEp, dEq = dp0 + dp3 < side, dq0 + dq3 < side
    # strong filter: three samples each side, each within 2 tC of what it was
    sp = [(p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, (p2 + p1 + p0 + q0 + 2) >> 2, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3]
    sq = [(p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3, (p0 + q0 + q1 + q2 + 2) >> 2, (p0 + q0 + q1 + 3 * q2 + 2 * q3 + 4) >> 3]
    spc = [np.clip(s, a - 2 * tC, a + 2 * tC) for s, a in zip(sp, (p0, p1, p2))]
    sqc = [np.clip(s, a - 2 * tC, a + 2 * tC) for s, a in zip(sq, (q0, q1, q2))]
    # normal filter: a line is left alone if its step is 10 tC or more
    delta0 = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4
    line = normal & (abs(delta0) < 10 * tC)
    delta = np.clip(delta0, -tC, tC)
    np0, nq0 = p0 + delta, q0 - delta
    dp1_0, dq1_0 = (((p2 + p0 + 1) >> 1) - p1 + delta) >> 1, (((q2 + q0 + 1) >> 1) - q1 - delta) >> 1
    dp1, dq1 = np.clip(dp1_0, -(tC >> 1), tC >> 1), np.clip(dq1_0, -(tC >> 1), tC >> 1)
    np1, nq1 = p1 + dp1, q1 + dq1
    sP, sQ, lP, lQ = strong & onP, strong & onQ, line & onP, line & onQ
    o = v.copy()
    o[..., 3] = np.where(sP, spc[0], np.where(lP, np.clip(np0, 0, mx), p0))
    o[..., 2] = np.where(sP, spc[1], np.where(lP & dEp, np.clip(np1, 0, mx), p1))
    o[..., 1] = np.where(sP, spc[2], p2)
    o[..., 4] = np.where(sQ, sqc[0], np.where(lQ, np.clip(nq0, 0, mx), q0))
    o[..., 5] = np.where(sQ, sqc[1], np.where(lQ & dEq, np.clip(nq1, 0, mx), q1))
    o[..., 6] = np.where(sQ, sqc[2], q2)
    P[:, 4:-4] = o.reshape(P.shape[0], (n_ac - 1) * 8)
    if tags is None:
        return
    n = lambda m: int(np.broadcast_to(m, v.shape[:4]).any(axis=2).sum())      # segments with the branch on any of their four lines

    def put(k, m):
        tags[f"{name}.luma.{k}"] += n(m)
    put("bS1", bS == 1)
    put("bS2", bS == 2)
    put("beta_exit", active & ~passed)
    put("tc0", passed & (tC == 0))
    for e, m in _en(onP, onQ):
        put("strong_" + e, strong & m)
        for a in (0, 1):
            for b in (0, 1):
                put(f"normal_{e}_dEp{a}_dEq{b}", normal & m & (dEp == bool(a)) & (dEq == bool(b)))
    s_clip = (sP & ((sp[0] != spc[0]) | (sp[1] != spc[1]) | (sp[2] != spc[2]))) | (sQ & ((sq[0] != sqc[0]) | (sq[1] != sqc[1]) | (sq[2] != sqc[2])))
    skipped = normal & (tC > 0) & ~line
    d_clip = (lP | lQ) & (delta != delta0)
    p_clip, q_clip = lP & dEp & (dp1 != dp1_0), lQ & dEq & (dq1 != dq1_0)
    put("strong_clipped", s_clip)
    put("line_skipped_10tc", skipped)
    put("line_skipped_big_tc", skipped & (tC >= 4 * sc))
    put("delta_clipped", d_clip)
    put("p1_clipped", p_clip)
    put("q1_clipped", q_clip)
    put("clip_lo", (lP & (np0 < 0)) | (lQ & (nq0 < 0)) | (lP & dEp & (np1 < 0)) | (lQ & dEq & (nq1 < 0)))
    put("clip_hi", (lP & (np0 > mx)) | (lQ & (nq0 > mx)) | (lP & dEp & (np1 > mx)) | (lQ & dEq & (nq1 > mx)))
    limited = np.broadcast_to(s_clip | d_clip | p_clip | q_clip, v.shape[:4]).any(axis=2, keepdims=True)
    for key, idx, m in (("beta_idx", bidx, passed), ("tc_idx", tidx, passed), ("tc_clip_idx", tidx, limited)):
        for i, c in enumerate(np.bincount(idx[m], minlength=54)):
            if c:
                tags[f"{name}.luma.{key}.{i}"] += int(c)


def _chroma_pass(C, bs0, qp, on, tc2, offset, bd, tags, name):
    """the chroma edges across the second axis of C, in place: on the 8-sample chroma grid, strength 2 only, position 0's strength for the
    whole segment, one sample each side"""
    n_al, n_ac = C.shape[0] // 4, C.shape[1] // 4
    xs = np.arange(2, n_ac, 2)
    if len(xs) == 0:
        return
    mx, sc = (1 << bd) - 1, 1 << (bd - 8)
    cols = 4 * xs
    get = lambda k: C[:, cols + k].reshape(n_al, 4, len(xs))
    p1, p0, q0, q1 = get(-2), get(-1), get(0), get(1)
    seg = lambda a: a[:, None, :]
    bS = seg(bs0[:n_al, xs])
    qPi = ((seg(qp[:n_al, xs]) + seg(qp[:n_al, xs - 1]) + 1) >> 1) + offset
    onP, onQ = seg(on[:n_al, xs - 1]), seg(on[:n_al, xs])
    qpc = np.where(qPi < 30, qPi, np.where(qPi > 42, qPi - 6, QPC_30_42[np.clip(qPi - 30, 0, 12)]))
    tidx = np.clip(qpc + 2 + (tc2 << 1), 0, 53)
    tC = TC[tidx] * sc
    f = bS == 2
    delta0 = (((q0 - p0) << 2) + p1 - q1 + 4) >> 3
    delta = np.clip(delta0, -tC, tC)
    np0, nq0 = p0 + delta, q0 - delta
    fP, fQ = f & onP, f & onQ
    C[:, cols - 1] = np.where(fP, np.clip(np0, 0, mx), p0).reshape(-1, len(xs))
    C[:, cols] = np.where(fQ, np.clip(nq0, 0, mx), q0).reshape(-1, len(xs))
    if tags is None:
        return
    n = lambda m: int(np.broadcast_to(m, p0.shape).any(axis=1).sum())

    def put(k, m):
        tags[f"{name}.{k}"] += n(m)
    for e, m in _en(onP, onQ):
        put(e, f & m)
    put("delta_clipped", (fP | fQ) & (delta != delta0))
    put("clip_lo", (fP & (np0 < 0)) | (fQ & (nq0 < 0)))
    put("clip_hi", (fP & (np0 > mx)) | (fQ & (nq0 > mx)))
    put("qpi_neg", f & (qPi < 0))
    put("qpi_0_29", f & (qPi >= 0) & (qPi < 30))
    put("qpi_30_42", f & (qPi >= 30) & (qPi <= 42))
    put("qpi_gt42", f & (qPi > 42))
    put("bs1_ignored", bS == 1)
    for i, c in enumerate(np.bincount(tidx[f], minlength=54)):
        if c:
            tags[f"{name}.tc_idx.{i}"] += int(c)


def restate(pic, tags=None):
    """-> [Y, Cb, Cr] after deblocking (2-D, picture size)"""
    W, H, bd = pic["W"], pic["H"], pic["bd"]
    gw, gh = (W + 63) // 64 * 8 + 1, (H + 63) // 64 * 8 + 1
    data, bs = pic["data"].reshape(gh, gw).astype(np.int64), pic["bs"].reshape(gh, gw).astype(np.int64)
    qp, on = data >> 1, (data & 1) == 0
    out = [pic[k].astype(np.int64) for k in ("y", "cb", "cr")]
    for e, name in enumerate(DIRS):
        t = (lambda a: a.T) if e else (lambda a: a)
        bs2 = [t((bs >> (4 * e + 2 * pos)) & 3) for pos in (0, 1)]
        _luma_pass(t(out[0]), bs2, t(qp), t(on), pic["tc2"], pic["beta2"], bd, tags, name)
        for c, off in ((1, pic["cbq"]), (2, pic["crq"])):
            _chroma_pass(t(out[c]), bs2[0], t(qp), t(on), pic["tc2"], off, bd, tags, f"{name}.{('cb', 'cr')[c - 1]}")
    return [o.astype(pic[k].dtype) for o, k in zip(out, ("y", "cb", "cr"))]


# ---- pictures ---------------------------------------------------------------------------------------------------------------------------
SIZES = ((64, 64), (72, 40), (208, 136), (136, 72), (8, 8), (8, 120), (104, 8), (24, 24), (200, 120), (88, 152), (16, 16), (120, 56))


def block_map(rng, W, H):
    """LoopFilter::Block arrays on the ((W + 63) / 64 * 8 + 1) x ((H + 63) / 64 * 8 + 1) grid, every entry drawn (those beyond the picture
    too: nothing may read them) except the strengths on the picture's left and top boundary, which are 0 as processCtu leaves them"""
    gw, gh = (W + 63) // 64 * 8 + 1, (H + 63) // 64 * 8 + 1
    data = ((rng.integers(0, 52, (gh, gw)) << 1) | (rng.random((gh, gw)) < 0.08)).astype(np.int8)
    bs = np.zeros((gh, gw), np.uint8)
    for k in range(4):
        bs |= (rng.integers(0, 3, (gh, gw)) << (2 * k)).astype(np.uint8)
    bs[:, 0] &= 0xF0
    bs[0, :] &= 0x0F
    return data.ravel(), bs.ravel()


def content(rng, h, w, bd, chroma=False):
    """8x8 blocks at a dark, middle or bright level one or two steps apart, most of them with noise: int64 [h, w]"""
    mx, sc = (1 << bd) - 1, 1 << (bd - 8)
    if chroma and rng.random() < 0.25:
        return rng.integers(0, 2, (h, w)) * mx                   # 0 / max "extremes": chroma has no dE gate
    amp, step = int(rng.choice([0, 1, 2, 4])) * sc, int(rng.choice([4, 12, 40, 100])) * sc
    level = int(rng.integers(0, 3))
    base, kmax = ((0, 1), ((mx - 2 * step) // 2, 2), (mx - step, 1))[level]
    nb = ((h + 7) // 8, (w + 7) // 8)
    grow = lambda a: np.kron(a, np.ones((8, 8), np.int64))[:h, :w]
    img = grow(base + rng.integers(0, kmax + 1, nb) * step)
    img = img + rng.integers(-amp, amp + 1, (h, w)) * grow((rng.random(nb) < 0.75).astype(np.int64))
    return np.clip(img, 0, mx)


def make_picture(seed, W=None, H=None, bd=None, S=None):
    """a seeded picture before deblocking: y / cb / cr (2-D, no padding), data / bs (the flat block map), tc2 / beta2 (the slice's
    tc_offset_div2 / beta_offset_div2), cbq / crq (pps_cb_qp_offset / pps_cr_qp_offset, never equal), W, H, bd, S"""
    rng = np.random.default_rng(seed)
    if W is None:
        W, H = SIZES[seed % len(SIZES)]
    bd = int(rng.choice([8, 8, 9, 10])) if bd is None else bd
    if S is None:
        S = 1 if bd == 8 and rng.integers(0, 3) else 2
    if rng.random() < 0.3:
        tc2, beta2 = int(rng.integers(-6, -2)), int(rng.integers(3, 7))
    else:
        tc2, beta2 = int(rng.integers(-6, 7)), int(rng.integers(-6, 7))
    cbq = int(rng.integers(-12, 13))
    crq = int(rng.choice([v for v in range(-12, 13) if v != cbq]))
    data, bs = block_map(rng, W, H)
    dt = np.uint8 if S == 1 else np.uint16
    y = content(rng, H, W, bd).astype(dt)
    cb, cr = (content(rng, H // 2, W // 2, bd, True).astype(dt) for _ in range(2))
    return dict(W=W, H=H, bd=bd, S=S, y=y, cb=cb, cr=cr, data=data, bs=bs, tc2=tc2, beta2=beta2, cbq=cbq, crq=crq)


def offsets(pic):
    return pic["tc2"], pic["beta2"], pic["cbq"], pic["crq"]


def run_cpu(impl, pic):
    """oracle.deblock / reference_c.deblock on a copy of the picture -> [Y, Cb, Cr]"""
    out = [pic[k].copy() for k in ("y", "cb", "cr")]
    impl.deblock(out[0], pic["W"], out[1], out[2], pic["W"] // 2, pic["W"], pic["H"], pic["bd"], pic["data"], pic["bs"], *offsets(pic))
    return out


def coverage(tags, floor=5):
    """-> (missing, summary): the names of `luma_tags()` / `chroma_tags()` reached fewer than `floor` times, the table indices not reached
    (luma beta 16..51, tc 18..53 and tC-limited tc 18..53 per direction, every reachable chroma tc index per direction and plane), and
    the minima as a line of text"""
    missing = [k for k in luma_tags() + chroma_tags() if tags[k] < floor]
    mins = {}
    for d in DIRS:
        for key, rng_ in (("beta_idx", range(16, 52)), ("tc_idx", range(18, 54)), ("tc_clip_idx", range(18, 54))):
            counts = [tags[f"{d}.luma.{key}.{i}"] for i in rng_]
            mins[f"{d}.luma.{key}"] = min(counts)
            missing += [f"{d}.luma.{key}.{i}" for i, c in zip(rng_, counts) if c < 1]
        for p in ("cb", "cr"):
            idx = sorted(chroma_tc_indices())
            counts = [tags[f"{d}.{p}.tc_idx.{i}"] for i in idx]
            mins[f"{d}.{p}.tc_idx"] = min(counts)
            missing += [f"{d}.{p}.tc_idx.{i}" for i, c in zip(idx, counts) if c < 1]
    rare = sorted(luma_tags() + chroma_tags(), key=lambda k: tags[k])[:6]
    summary = "rarest tags " + ", ".join(f"{k}={tags[k]}" for k in rare) + "; rarest table index per histogram " + ", ".join(f"{k}>={v}" for k, v in mins.items())
    return missing, summary


def new_tags():
    return collections.Counter()
