"""Generators, a numpy restatement and the layouts of tests/test_satd_paths.py: every Hadamard SATD path of the device (k_satd, k_satd_multi in its row and tile forms,
k_subpel_satd, k_intra_satd35, k_intra_measure) at its 16-bit bounds, on every tile form and in every launch class.  Nothing here computes an expected value: those come
from the `oracle` fixture in the test module.  What is here says WHICH inputs are adversarial, and the numpy restatement says what they reach.

A tile is a pair of n x n sample blocks (a, b), n = 8 / 4 / 2, with difference d = a - b; mx = 2^bitDepth - 1.
  walsh     a = mx where +-W(u, v) > 0, b the complement: +-n^2 mx on ONE coefficient (64 mx at 8x8), +-32 mx on a five-stage intermediate
  bent      d = mx (-1)^f, f = x0 x1 ^ x2 x3 ^ x4 x5 over the index bits (x0 x1 ^ x2 x3 at 4x4), its negation and its transpose: every coefficient 8 mx (4 mx at 4x4), the
            largest sum of magnitudes a tile can have
  impulse   one difference of +-mx, the rest 0 (a == b there, random): every position
  random    uniform, and random 0 / mx: the only ones whose sum is not a multiple of 4 (the rounding term of (sum + 2) >> 2)
  2x2       all 16 sign patterns of +-mx
The tiles are laid out as MOSAICS in two planes of different strides whose mosaic origins are at different odd sample offsets (unaligned packed loads, a's and b's
alignments differ): 256 8x8 tiles (mosaic rows 0 .. 127), 128 4x4 tiles (rows 128 .. 143), 256 2x2 tiles (rows 144 .. 151), each family shuffled so that a w x h job on
the grid of its tile kind covers w h / n^2 different family members.
"""
import numpy as np

import cases

BIT_DEPTHS = (8, 9, 10)
MARGIN = cases.PAD + 4        # every block AND its (w + 7) x (h + 7) interpolation window stays cases.PAD samples inside its buffer
MW, MH = 128, 152             # the mosaic, in samples
REGION = {8: (0, 128), 4: (128, 16), 2: (144, 8)}     # tile kind -> (first mosaic row, rows)
EXTRA_SHAPES = [(2, 2), (4, 4), (8, 8), (6, 8), (2, 4), (12, 8)]
SHAPES = sorted(set(cases.PU_SIZES) | set(cases.CHROMA_PU_SIZES) | set(EXTRA_SHAPES), key=lambda s: (-s[0] * s[1], -s[0]))
SENTINEL = -0x5a5a5a5b

# asserted literals (tests/test_satd_paths.py::test_family_constants): cost of a full-amplitude Walsh tile / of the bent tile at 8 / 9 / 10 bits
WALSH_COST = {8: 4080, 9: 2044, 10: 4092}
BENT_COST = {8: 32640, 9: 16352, 10: 32736}


def S_of(bd):
    return 1 if bd == 8 else 2


def dtype_of(bd):
    return cases.sample_dtype(S_of(bd))


def kind_of(w, h):
    """turing/Measure.h:97-135: 8x8 tiles when both sides are multiples of 8, else 4x4 when multiples of 4, else 2x2"""
    return 2 if (w | h) & 3 else 4 if (w | h) & 7 else 8


def fits(shape, max_w, max_h):
    return shape[0] <= max_w and shape[1] <= max_h


def shapes_of(max_w, max_h, taps=None):
    """every shape that fits the class; with 8 taps (luma) no width 2 or 6"""
    return [s for s in SHAPES if fits(s, max_w, max_h) and not (taps == 8 and s[0] in (2, 6))]


def hadamard(n):
    i = np.arange(n)
    return 1 - 2 * (np.array([[bin(u & x).count("1") for x in i] for u in i]) & 1)


# ================================================================================================================== numpy restatement
def np_tile_satd(d, S):
    """d: int array [..., n, n] of differences -> the tile costs (havoc/hadamard.cpp:58-98): sum of |H d H^T|, (s + 2) >> 2 at 8x8, (s + 1) >> 1 at 4x4, s at 2x2; the
    16-bit tables shift by two more"""
    d = np.asarray(d, np.int64)
    n = d.shape[-1]
    h = hadamard(n)
    s = np.abs(h @ d @ h.T).sum(axis=(-1, -2))
    s = (s + 2) >> 2 if n == 8 else (s + 1) >> 1 if n == 4 else s
    return s >> 2 if S == 2 else s


def np_tile_sum(d):
    """the sum of magnitudes before any normalisation"""
    d = np.asarray(d, np.int64)
    h = hadamard(d.shape[-1])
    return np.abs(h @ d @ h.T).sum(axis=(-1, -2))


def np_pu_satd(a, b, S):
    """a, b: [h, w] blocks -> the PU SATD (turing/Measure.h:97-135)"""
    h, w = a.shape
    n = kind_of(w, h)
    d = np.asarray(a, np.int64) - np.asarray(b, np.int64)
    return int(np_tile_satd(d.reshape(h // n, n, w // n, n).transpose(0, 2, 1, 3), S).sum())


def np_stage_peaks(d):
    """d: [..., 8, 8] -> the largest magnitude after each of the six butterfly stages of the 64-point transform, in the order of the tile-per-lane kernels: the five
    stages between registers (index bits 1 .. 5) first, the one inside a register (bit 0: the two samples of a pair) last"""
    v = np.asarray(d, np.int64).reshape(d.shape[:-2] + (64,))
    peaks = []
    for bit in (1, 2, 3, 4, 5, 0):
        t = v.reshape(v.shape[:-1] + (64 >> (bit + 1), 2, 1 << bit))
        v = np.stack([t[..., 0, :] + t[..., 1, :], t[..., 0, :] - t[..., 1, :]], axis=-2).reshape(v.shape)
        peaks.append(int(np.abs(v).max()))
    return peaks


# ================================================================================================================== the families
def walsh_tiles(n, mx):
    h = hadamard(n)
    out = []
    for u in range(n):
        for v in range(n):
            for sign in (1, -1):
                a = np.where(sign * np.outer(h[u], h[v]) > 0, mx, 0)
                out.append((("walsh", u, v, sign), a, mx - a))
    return out


def bent_difference(n):
    """(-1)^f over the index bits of y * n + x: f = x0 x1 ^ x2 x3 ^ x4 x5 (8x8), x0 x1 ^ x2 x3 (4x4)"""
    idx = np.arange(n * n)
    f = 0
    for k in range(0, 2 * (n.bit_length() - 1), 2):
        f = f ^ ((idx >> k) & (idx >> (k + 1)) & 1)
    return (1 - 2 * f).reshape(n, n)


def bent_tiles(n, mx):
    s = bent_difference(n)
    return [(("bent", name), np.where(d > 0, mx, 0), np.where(d < 0, mx, 0)) for name, d in (("plain", s), ("negated", -s), ("transposed", s.T))]


def impulse_tiles(n, mx, rng):
    out = []
    for pos in range(n * n):
        sign = 1 if bin(pos).count("1") % 2 == 0 else -1
        a = rng.integers(0, mx + 1, (n, n))
        b = a.copy()
        a[pos // n, pos % n], b[pos // n, pos % n] = (mx, 0) if sign > 0 else (0, mx)
        out.append((("impulse", pos, sign), a, b))
    return out


def random_tiles(n, mx, rng, count):
    out = []
    for i in range(count):
        a, b = (rng.integers(0, 2, (2, n, n)) * mx) if i & 1 else rng.integers(0, mx + 1, (2, n, n))
        out.append((("random", "extremes" if i & 1 else "uniform", i), a, b))
    return out


def sign_tiles_2x2(mx):
    out = []
    for m in range(16):
        d = np.array([1 if m >> k & 1 else -1 for k in range(4)]).reshape(2, 2)
        out.append((("signs", m), np.where(d > 0, mx, 0), np.where(d < 0, mx, 0)))
    return out


def family(n, bd, seed=5):
    """the tiles of kind n in mosaic order (shuffled): 256 / 128 / 256 of them"""
    mx = (1 << bd) - 1
    rng = np.random.default_rng(seed + 10 * n + bd)
    if n == 2:
        tiles = sign_tiles_2x2(mx) + random_tiles(2, mx, rng, 240)
    else:
        tiles = walsh_tiles(n, mx) + bent_tiles(n, mx) + impulse_tiles(n, mx, rng)
        tiles += random_tiles(n, mx, rng, (256 if n == 8 else 128) - len(tiles))
    return [tiles[i] for i in rng.permutation(len(tiles))]


class Mosaic:
    """the two planes: `a` (stride sa, mosaic origin (ax, ay)) and `b` (stride sb, origin (bx, by)); tags[n][gy][gx] names the tile at grid cell (gx, gy) of kind n"""
    sa, sb = 171, 174
    ax, ay, bx, by = MARGIN + 1, MARGIN + 3, MARGIN + 3, MARGIN + 1

    def __init__(self, bd):
        self.bd, self.S, self.mx = bd, S_of(bd), (1 << bd) - 1
        rng = np.random.default_rng(40 + bd)
        dt = dtype_of(bd)
        a = rng.integers(0, self.mx + 1, (self.ay + MH + MARGIN, self.sa))
        b = rng.integers(0, self.mx + 1, (self.by + MH + MARGIN, self.sb))
        self.tags, self.tiles = {}, {}
        for n, (y0, rows) in REGION.items():
            per_row = MW // n
            fam = family(n, bd)
            assert len(fam) == per_row * (rows // n)
            self.tiles[n] = fam
            self.tags[n] = [[fam[gy * per_row + gx][0] for gx in range(per_row)] for gy in range(rows // n)]
            for i, (_, ta, tb) in enumerate(fam):
                x, y = (i % per_row) * n, y0 + (i // per_row) * n
                a[self.ay + y:self.ay + y + n, self.ax + x:self.ax + x + n] = ta
                b[self.by + y:self.by + y + n, self.bx + x:self.bx + x + n] = tb
        self.a, self.b = np.ascontiguousarray(a.astype(dt)).ravel(), np.ascontiguousarray(b.astype(dt)).ravel()

    def a_off(self, x, y):
        return (self.ay + y) * self.sa + self.ax + x

    def b_off(self, x, y):
        return (self.by + y) * self.sb + self.bx + x

    def block_a(self, x, y, w, h):
        return self.a.reshape(-1, self.sa)[self.ay + y:self.ay + y + h, self.ax + x:self.ax + x + w]

    def block_b(self, x, y, w, h):
        return self.b.reshape(-1, self.sb)[self.by + y:self.by + y + h, self.bx + x:self.bx + x + w]

    def tags_under(self, x, y, w, h):
        n = kind_of(w, h)
        y0 = REGION[n][0]
        return [self.tags[n][(y - y0) // n + j][x // n + i] for j in range(h // n) for i in range(w // n)]


_mosaics = {}


def mosaic(bd):
    if bd not in _mosaics:
        _mosaics[bd] = Mosaic(bd)
    return _mosaics[bd]


# ================================================================================================================== jobs on the mosaic grid
def grid_positions(w, h):
    """the mosaic of the shape's tile kind tiled by the shape: [(x, y)] in mosaic samples"""
    y0, rows = REGION[kind_of(w, h)]
    return [(x, y0 + y) for y in range(0, rows - h + 1, h) for x in range(0, MW - w + 1, w)]


def candidate_position(w, h, x, y, k):
    """the k-th of 16 DISTINCT positions of a w x h block on the grid of its kind; k = 0 is (x, y) itself"""
    n = kind_of(w, h)
    y0, rows = REGION[n]
    cx, cy = (MW - w) // n + 1, (rows - h) // n + 1
    total = cx * cy
    assert total >= 16
    step = next(s for s in (7, 11, 13, 17, 19, 1) if np.gcd(s, total) == 1)
    p = (((y - y0) // n) * cx + x // n + k * step) % total
    return (p % cx) * n, y0 + (p // cx) * n


def shuffled(rows, seed):
    rows = np.asarray(rows, np.int32)
    return np.ascontiguousarray(rows[np.random.default_rng(seed).permutation(len(rows))])


def pair_jobs(bd, max_w, max_h, seed=1):
    """havoc_mi355x_pair_job rows (a_off, b_off, w, h) with the shape's (x, y) kept beside them: every shape that fits, each tiled over the mosaic (a and b at the same
    cell: the adversarial differences), shuffled.  -> (jobs int32 [n, 4], cells [n, 4] = x, y, w, h)"""
    m = mosaic(bd)
    rows = [(m.a_off(x, y), m.b_off(x, y), w, h, x, y) for (w, h) in shapes_of(max_w, max_h) for (x, y) in grid_positions(w, h)]
    rows = shuffled(rows, seed + 100 * max_w + max_h)
    return np.ascontiguousarray(rows[:, :4]), rows[:, [4, 5, 2, 3]]


def multi_jobs(bd, max_w, max_h, seed=2):
    """havoc_mi355x_satd_multi_job rows (a_off, w, h, count, b_off[16]): as pair_jobs, candidate 0 the block's own cell and candidates 1 .. 15 fifteen other cells; count
    cycles through 1 .. 16 AFTER the shuffle, so the first 16 jobs of a launch hold every count; all 16 b_off are in range whatever the count"""
    m = mosaic(bd)
    rows = []
    for (w, h) in shapes_of(max_w, max_h):
        for (x, y) in grid_positions(w, h):
            rows.append([m.a_off(x, y), w, h, 0] + [m.b_off(*candidate_position(w, h, x, y, k)) for k in range(16)] + [x, y])
    rows = shuffled(rows, seed + 100 * max_w + max_h)
    rows[:, 3] = 1 + np.arange(len(rows)) % 16
    return np.ascontiguousarray(rows[:, :20]), rows[:, [20, 21, 1, 2]]


def label(cells, i):
    x, y, w, h = (int(v) for v in cells[i])
    return f"job {i}: {w}x{h} at mosaic ({x}, {y})"


# ================================================================================================================== part C: planes and jobs of the fused kernel
SUBPEL_CLASSES = (8, 16, 32, 64)
SUBPEL_JOBS_PER_WORKGROUP = {8: 32, 16: 8, 32: 2, 64: 1}
# (ii): per class one 8x8-tiled shape, one 4x4-tiled one and, with 4 taps, one 2x2-tiled one
SUBPEL_PHASE_SHAPES = {8: [(8, 8), (4, 8), (6, 8)], 16: [(16, 16), (12, 16), (8, 6)], 32: [(32, 32), (16, 12), (2, 4)], 64: [(64, 64), (16, 4), (8, 2)]}
SUBPEL_W, SUBPEL_H = 177, 176          # the reference plane of (ii)
SUBPEL_SW = 169                        # the source plane's stride


def phases(taps):
    n = 4 if taps == 8 else 8
    return [(xf, yf) for yf in range(n) for xf in range(n)]


def step_plane(bd):
    """0 / mx only: 24 x 24 cells of stripes (4 wide, 1 wide, vertical and horizontal), checkerboards (1 x 1, 2 x 2) and irregular steps -- every filter overshoots at
    their edges, below 0 and above mx"""
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:SUBPEL_H, 0:SUBPEL_W]
    cell = ((yy // 24) * 3 + xx // 24) % 6
    pats = [(xx // 4) & 1, (yy // 4) & 1, (xx + yy) & 1, ((xx // 2) + (yy // 2)) & 1, xx & 1, (yy // 3 + xx // 5) & 1]
    p = np.zeros_like(xx)
    for k, q in enumerate(pats):
        p = np.where(cell == k, q, p)
    return np.ascontiguousarray((p * mx).astype(dtype_of(bd))).ravel()


_planes = {}


def subpel_planes(bd, kind):
    """(source plane, stride, reference plane, stride): kind "uniform" or "steps" (the source of "steps" is random 0 / mx)"""
    if (bd, kind) not in _planes:
        rng = np.random.default_rng(70 + bd + (100 if kind == "steps" else 0))
        mx = (1 << bd) - 1
        if kind == "uniform":
            src, ref = rng.integers(0, mx + 1, SUBPEL_H * SUBPEL_SW), rng.integers(0, mx + 1, SUBPEL_H * SUBPEL_W)
            src, ref = src.astype(dtype_of(bd)), ref.astype(dtype_of(bd))
        else:
            src, ref = (rng.integers(0, 2, SUBPEL_H * SUBPEL_SW) * mx).astype(dtype_of(bd)), step_plane(bd)
        _planes[bd, kind] = (np.ascontiguousarray(src), SUBPEL_SW, np.ascontiguousarray(ref), SUBPEL_W)
    return _planes[bd, kind]


def subpel_phase_jobs(taps, cls, seed=3, per_shape=3):
    """havoc_mi355x_pred_uni_job rows (src_off, ref_off, w, h, xFrac, yFrac, 0, 0): every phase pair x the class's shapes x `per_shape` positions whose windows stay
    MARGIN - 4 >= cases.PAD inside the planes"""
    rng = np.random.default_rng(seed + 10 * cls + taps)
    rows = []
    for (xf, yf) in phases(taps):
        for (w, h) in SUBPEL_PHASE_SHAPES[cls][:3 if taps == 4 else 2]:
            for _ in range(per_shape):
                sx, sy = (int(rng.integers(MARGIN, lim - MARGIN - s + 1)) for lim, s in ((SUBPEL_SW, w), (SUBPEL_H, h)))
                rx, ry = (int(rng.integers(MARGIN, lim - MARGIN - s + 1)) for lim, s in ((SUBPEL_W, w), (SUBPEL_H, h)))
                rows.append((sy * SUBPEL_SW + sx, ry * SUBPEL_W + rx, w, h, xf, yf, 0, 0))
    return shuffled(rows, seed + cls)


def subpel_mosaic_jobs(bd, taps, cls, seed=4):
    """(i): phase (0, 0) over the mosaics, source = plane a, reference = plane b at the same cell: the prediction is the block of b itself"""
    m = mosaic(bd)
    rows = [(m.a_off(x, y), m.b_off(x, y), w, h, 0, 0, 0, 0) for (w, h) in shapes_of(cls, cls, taps) for (x, y) in grid_positions(w, h)]
    return shuffled(rows, seed + cls + taps)


LUMA_TAPS = np.array([[0, 0, 0, 64, 0, 0, 0, 0], [-1, 4, -10, 58, 17, -5, 1, 0], [-1, 4, -11, 40, 40, -11, 4, -1], [0, 1, -5, 17, 58, -10, 4, -1]])
CHROMA_TAPS = np.array([[0, 64, 0, 0], [-2, 58, 10, -2], [-4, 54, 16, -2], [-6, 46, 28, -4], [-4, 36, 36, -4], [-4, 28, 46, -6], [-2, 16, 54, -4], [-2, 10, 58, -2]])


def np_pred_uni_unclipped(ref, stride, off, w, h, xf, yf, bd, taps):
    """the HEVC fractional-sample interpolation (8.5.3.3.3) BEFORE its final clip, two passes as the device makes them: [h, w] int64"""
    c = LUMA_TAPS if taps == 8 else CHROMA_TAPS
    ab = taps // 2 - 1
    p = np.asarray(ref, np.int64).reshape(-1, stride)
    y0, x0 = divmod(off, stride)
    win = p[y0 - ab:y0 - ab + h + taps - 1, x0 - ab:x0 - ab + w + taps - 1]
    t = sum(c[xf][k] * win[:, k:k + w] for k in range(taps)) >> min(4, bd - 8)
    v = sum(c[yf][k] * t[k:k + h] for k in range(taps))
    shift = 6 + max(2, 14 - bd)
    return (v + (1 << (shift - 1))) >> shift


# ================================================================================================================== part D: the two intra stages
NB_LEN, NB_CENTRE = 160, 80          # one neighbour array and the index of neighbours[0] = p(0, -1) in it (cases.rand_neighbours)


def pack_blocks(blocks, dt, stride, x0, y0, rng, mx):
    """n x n blocks side by side in a random plane of that stride, first block at (x0, y0) -> (flat plane, offset of each block)"""
    n = blocks[0].shape[0]
    per_row = (stride - x0 - cases.PAD) // n
    rows = -(-len(blocks) // per_row)
    plane = rng.integers(0, mx + 1, (y0 + rows * n + cases.PAD, stride))
    offs = []
    for i, blk in enumerate(blocks):
        y, x = y0 + (i // per_row) * n, x0 + (i % per_row) * n
        plane[y:y + n, x:x + n] = blk
        offs.append(y * stride + x)
    return np.ascontiguousarray(plane.astype(dt)).ravel(), offs


def intra_case(bd, log2):
    """-> dict(src, ss, nb, jobs int32 [n, 8] = (src_off, nb_off, nbf_off, filt_lo, filt_hi, edge, log2, 0), tags)
      half      source = (n / ts)^2 half-amplitude tiles mx (1 +- W) / 2; neighbours flat 0 (mask 0, edge on) and flat mx (mask all ones, edge off): every mode predicts flat
      top / left  edge 0: mode 26 copies the row above down each column, mode 10 the left column along each row; the row (column) holds a 0 / mx Walsh pattern of period ts
                and the source its complement: full amplitude on the ts + ts separable patterns, both signs, the pattern in the unfiltered array (mask 0) and in the
                filtered one (mask all ones)
      random    uniform and 0 / mx sources and neighbours, a random mask and its complement, edge on and off"""
    n, mx, dt = 1 << log2, (1 << bd) - 1, dtype_of(bd)
    ts = min(n, 8)
    k = n // ts
    rng = np.random.default_rng(900 + 10 * bd + log2)
    h = hadamard(ts)
    blocks, specs = [], []      # spec: (tag, nb array, nbf array, mask, edge)
    flat0, flat1 = np.zeros(NB_LEN, np.int64), np.full(NB_LEN, mx)
    ALL = (1 << 35) - 1

    halves = [t[1] for t in walsh_tiles(ts, mx)]
    for i in range(0, len(halves), k * k):
        blk = np.block([[halves[i + r * k + c] for c in range(k)] for r in range(k)])
        for nb, mask, edge in ((flat0, 0, 1), (flat1, ALL, 0)):
            blocks.append(blk)
            specs.append((("half", i // (k * k), int(nb[0] != 0)), nb, nb, mask, edge))
    for v in range(ts):
        for sign in (1, -1):
            pat = np.where(sign * h[v][np.arange(2 * n) % ts] > 0, mx, 0)
            for where in ("top", "left"):
                line = rng.integers(0, mx + 1, NB_LEN)
                if where == "top":
                    line[NB_CENTRE:NB_CENTRE + 2 * n] = pat                                       # p(x, -1) = neighbours[x]
                    blk = np.tile(mx - pat[:n], (n, 1))
                else:
                    line[NB_CENTRE - 2 - np.arange(2 * n)] = pat                                  # p(-1, y) = neighbours[-2 - y]
                    blk = np.tile((mx - pat[:n])[:, None], (1, n))
                other = rng.integers(0, mx + 1, NB_LEN)
                for nb, nbf, mask in ((line, other, 0), (other, line, ALL)):
                    blocks.append(blk)
                    specs.append(((where, v, sign, int(mask != 0)), nb, nbf, mask, 0))
    for i in range(4):
        blk = rng.integers(0, 2, (n, n)) * mx if i & 1 else rng.integers(0, mx + 1, (n, n))
        nb, nbf = (rng.integers(0, 2, (2, NB_LEN)) * mx) if i & 2 else rng.integers(0, mx + 1, (2, NB_LEN))
        mask = int(rng.integers(0, 1 << 35))
        for msk in (mask, ALL ^ mask):
            blocks.append(blk)
            specs.append((("random", i, int(msk == mask)), nb, nbf, msk, i & 1))

    src, offs = pack_blocks(blocks, dt, 173, cases.PAD + 1, cases.PAD + 3, rng, mx)
    nbs, jobs = [], []
    for off, (tag, nb, nbf, mask, edge) in zip(offs, specs):
        base = NB_LEN * len(nbs)
        nbs += [nb, nbf]
        jobs.append((off, base + NB_CENTRE, base + NB_LEN + NB_CENTRE, mask & 0xffffffff, mask >> 32, edge, log2, 0))
    return dict(src=src, ss=173, nb=np.ascontiguousarray(np.concatenate(nbs).astype(dt)), tags=[s[0] for s in specs],
                jobs=np.array(jobs, np.int64).astype(np.uint32).view(np.int32).reshape(len(jobs), 8))


def measure_jobs(bd, log2):
    """havoc_mi355x_tu_fused_job rows (coef_off, src_off, pred_off, rec_off) of intra_measure over the mosaics: source = plane a, prediction = plane b; every cell of the
    n x n tiling with the prediction at the same cell (full amplitude) and once more with the prediction at another cell.  -> (jobs, cells)"""
    m = mosaic(bd)
    n = 1 << log2
    rows = []
    for k in (0, 5):
        for (x, y) in grid_positions(n, n):
            rows.append((0, m.a_off(x, y), m.b_off(*candidate_position(n, n, x, y, k)), 0, x, y, n, n))
    rows = shuffled(rows, 6 + log2)
    rows[:, 0] = rows[:, 3] = np.arange(len(rows)) * n * n
    return np.ascontiguousarray(rows[:, :4]), rows[:, 4:]
