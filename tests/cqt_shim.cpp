// TEST INFRASTRUCTURE ONLY.  The reference's own bits of a coding quadtree: Syntax<coding_quadtree>::go (turing/SyntaxCtu.hpp:95-139) driven over a small stand-in
// handle whose tag is Measure<void>, so that split_cu_flag goes to the reference's own writer -- Write<Element<split_cu_flag, ae>> (turing/Binarization.h:102-122) --
// and its bin to Measure<EncodeDecision> (turing/Write.h:494-506), the measureEncodeDecision of the context-updating EstimateRate.  Compiled with oracle/Makefile's
// TURFLAGS into a temporary directory by tests/cqt_tools.py; nothing of the reference is stored.
//
// The stand-in holds a real ContextsAndCost, the current coding_quadtree, and a real Neighbourhood over a real StateSpatial: the snake is sized by the reference's
// StateSpatial::resize, reset as preCtu resets it at a slice's first CTU (turing/StatePictures.h:1086-1101: foreach over the upper row and the left column,
// BlockData::reset) and written only through the reference's own commitRectangle with BlockData::setup.
//
// Stubs: h(coding_quadtree) makes the node the current one and runs the reference's Syntax<coding_quadtree>::go on it (what Write<coding_quadtree> does around its
// extras); h(coding_unit) adds the node's supplied rate and commits the unit's CtDepth; h(Deleted<coding_quadtree>) does nothing, as in Search (turing/Search.hpp:
// 608-640 touches the sample snakes only).  split_cu_flag's VALUE is the caller's: one given value (cqt_flag), or "the decided CtDepth at (x0, y0) is deeper than this
// node" over a given final depth map -- the encoder's own rule when it walks the decided tree again (turing/Write.h:806-812).
#include "turing/StateEncode.h"
#include "turing/EstimateRate.h"
#include "turing/Measure.h"
#include "turing/StateSpatial.h"
#include "turing/SyntaxCtu.hpp"
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace {

template <class Tag, class F> struct Rebind;
template <template <class> class Verb, class F> struct Rebind<Verb<void>, F> { typedef Verb<F> type; };

struct State
{
    ContextsAndCost cc;
    coding_quadtree cqt;
    StateSpatial spatial;
    Neighbourhood nb;
    int W, H, ctbLog2, minCbLog2;
    int flagValue;                  // cqt_flag: the value to code
    const int8_t *finalDepth;       // cqt_ctu: the decided CtDepth per MinCb cell, rows `stride` apart
    int stride, xCtb, yCtb;
    const int64_t *nodeRate;        // cqt_ctu: the Q16 rate of the coding unit at each node of the CTU
    int scratch;
    State() : cqt(0, 0, 3, 0), finalDepth(nullptr), nodeRate(nullptr) {}
};

alignas(64) char nobody[1 << 16];

struct Handle
{
    typedef Measure<void> Tag;
    State *st;

    // ---- the stubs
    void operator()(coding_quadtree cqt)
    {
        st->cqt = cqt;
        Syntax<coding_quadtree>::go(cqt, *this);
    }
    void operator()(coding_unit cu)
    {
        const int d = st->ctbLog2 - cu.log2CbSize, cx = (cu.x0 - st->xCtb) >> cu.log2CbSize, cy = (cu.y0 - st->yCtb) >> cu.log2CbSize;
        int z = 0;
        for (int b = 0; b < d; ++b) z |= (cx >> b & 1) << (2 * b) | (cy >> b & 1) << (2 * b + 1);
        if (st->nodeRate) st->cc.rate.value += st->nodeRate[((1 << (2 * d)) - 1) / 3 + z];
        const coding_quadtree node(cu.x0, cu.y0, cu.log2CbSize, d);
        BlockData blockData;
        blockData.setup(&node, MODE_INTER);
        const int size = 1 << cu.log2CbSize;
        st->nb.snake.commitRectangle(Turing::Rectangle{ cu.x0, cu.y0, size, size }, blockData, st->nb.MinCbLog2SizeYMinus1);
    }
    template <class Direction> void operator()(Deleted<coding_quadtree, Direction>) { }
    // ---- everything else by the tag
    template <class V, class M> void operator()(V v, M m) { Rebind<Tag, Element<V, M>>::type::go(Element<V, M>{ v, m }, *this); }
    template <class F> void operator()(F f) { Rebind<Tag, F>::type::go(f, *this); }

    // ---- values
    int operator[](pic_width_in_luma_samples) const { return st->W; }
    int operator[](pic_height_in_luma_samples) const { return st->H; }
    int operator[](MinCbLog2SizeY) const { return st->minCbLog2; }
    int operator[](CtbLog2SizeY) const { return st->ctbLog2; }
    int operator[](PicWidthInCtbsY) const { return (st->W + (1 << st->ctbLog2) - 1) >> st->ctbLog2; }
    int operator[](PicHeightInCtbsY) const { return (st->H + (1 << st->ctbLog2) - 1) >> st->ctbLog2; }
    int operator[](cu_qp_delta_enabled_flag) const { return 0; }
    int operator[](cu_chroma_qp_offset_enabled_flag) const { return 0; }
    int operator[](Log2MinCuQpDeltaSize) const { return 0; }
    int operator[](Log2MinCuChromaQpOffsetSize) const { return 0; }
    int &operator[](IsCuQpDeltaCoded) { return st->scratch; }
    int &operator[](CuQpDeltaVal) { return st->scratch; }
    int &operator[](IsCuChromaQpOffsetCoded) { return st->scratch; }
    int operator[](split_cu_flag v) const
    {
        if (!st->finalDepth) return st->flagValue;
        return st->finalDepth[(v.y0 >> st->minCbLog2) * st->stride + (v.x0 >> st->minCbLog2)] > st->cqt.cqtDepth;
    }

    // ---- state
    operator coding_quadtree *() { return &st->cqt; }
    operator const coding_quadtree *() { return &st->cqt; }
    operator Contexts *() { return &st->cc; }
    operator StateEstimateRate *() { return &st->cc; }
    operator Neighbourhood *() { return &st->nb; }
    operator StateSpatial *() { return &st->spatial; }
    template <class T> operator T *() { return reinterpret_cast<T *>(nobody); }
};

State *open(int W, int H, int ctbLog2, int minCbLog2)
{
    State *st = new State();
    st->W = W, st->H = H, st->ctbLog2 = ctbLog2, st->minCbLog2 = minCbLog2;
    Handle h{ st };
    st->spatial.resize(h, st->nb);
    // the slice's first CTU (StatePictures.h:1086-1101)
    Turing::Rectangle rectangle;
    rectangle.x0 = 0;
    rectangle.y0 = 0;
    rectangle.width = h[PicWidthInCtbsY()] << ctbLog2;
    rectangle.height = h[PicHeightInCtbsY()] << ctbLog2;
    st->nb.snake.foreach(rectangle, minCbLog2 - 1, 1, 1, [](BlockData &data) { data.reset(); });
    return st;
}

void commit(State *st, int x0, int y0, int size, int depth)
{
    const coding_quadtree node(x0, y0, 0, depth);
    BlockData blockData;
    blockData.setup(&node, MODE_INTER);
    st->nb.snake.commitRectangle(Turing::Rectangle{ x0, y0, size, size }, blockData, st->nb.MinCbLog2SizeYMinus1);
}

void put(Contexts &c, const uint8_t *s) { for (int i = 0; i < 3; ++i) c.get<split_cu_flag>(i).state = s[i]; }
void take(Contexts &c, uint8_t *s) { for (int i = 0; i < 3; ++i) s[i] = c.get<split_cu_flag>(i).state; }

} // namespace

template <> struct SampleType<Handle> { typedef uint8_t Type; };

// what the snake answers after the slice-start reset, nothing committed: out[0] = CtDepth left of (x, y), out[1] = CtDepth above (x, y) -- as the writer reads them
extern "C" void cqt_snake_after_reset(int W, int H, int ctbLog2, int minCbLog2, int x, int y, int32_t *out)
{
    State *st = open(W, H, ctbLog2, minCbLog2);
    out[0] = st->nb.snake.get<Left>(x - 1, y, st->nb.MinCbLog2SizeYMinus1).CtDepth;
    out[1] = st->nb.snake.get<Up>(x, y - 1, st->nb.MinCbLog2SizeYMinus1).CtDepth;
    delete st;
}

// one split_cu_flag by the reference's writer.  p: int32 [11] = W, H, CtbLog2SizeY, MinCbLog2SizeY, x0, y0, log2CbSize, cqtDepth, the left neighbour's CtDepth, the upper
// neighbour's (each the depth of a MinCb unit committed at that place, or -1: nothing is committed there), binVal; states: split_cu_flag's three contexts, updated in
// place; out: int32 [3] = ctxInc (the context that moved), CtDepth the snake answered left, above -> the Q16 rate
extern "C" int64_t cqt_flag(const int32_t *p, uint8_t *states, int32_t *out)
{
    State *st = open(p[0], p[1], p[2], p[3]);
    const int x0 = p[4], y0 = p[5], minCb = 1 << p[3];
    if (p[9] >= 0) commit(st, x0, y0 - minCb, minCb, p[9]);
    if (p[8] >= 0) commit(st, x0 - minCb, y0, minCb, p[8]);
    st->cqt = coding_quadtree(x0, y0, p[6], p[7]);
    st->flagValue = p[10];
    put(st->cc, states);
    uint8_t before[3];
    take(st->cc, before);
    st->cc.rate = Cost();
    Handle h{ st };
    out[1] = st->nb.snake.get<Left>(x0 - 1, y0, st->nb.MinCbLog2SizeYMinus1).CtDepth;
    out[2] = st->nb.snake.get<Up>(x0, y0 - 1, st->nb.MinCbLog2SizeYMinus1).CtDepth;
    h(split_cu_flag(x0, y0), ae(v));
    take(st->cc, states);
    out[0] = -1;
    for (int i = 0; i < 3; ++i)
        if (states[i] != before[i]) out[0] = i;
    const int64_t rate = st->cc.rate.value;
    delete st;
    return rate;
}

// a picture walked CTU by CTU in coding order over its decided tree: the snake lives from cqt_open to cqt_close
extern "C" void *cqt_open(int W, int H, int ctbLog2, int minCbLog2) { return open(W, H, ctbLog2, minCbLog2); }
extern "C" void cqt_close(void *s) { delete static_cast<State *>(s); }
// a refused CTU's cells: CtDepth `depth` over size x size at (x0, y0), without any syntax
extern "C" void cqt_commit(void *s, int x0, int y0, int size, int depth) { commit(static_cast<State *>(s), x0, y0, size, depth); }
// Syntax<coding_quadtree>::go of the CTU at (xCtb, yCtb) with split_cu_flag from finalDepth (the picture's decided CtDepth per MinCb cell, rows `stride` apart);
// nodeRate: the coding unit's Q16 rate per node of the CTU; states updated in place -> the Q16 rate of the CTU
extern "C" int64_t cqt_ctu(void *s, int xCtb, int yCtb, uint8_t *states, const int8_t *finalDepth, int stride, const int64_t *nodeRate)
{
    State *st = static_cast<State *>(s);
    st->finalDepth = finalDepth, st->stride = stride, st->nodeRate = nodeRate, st->xCtb = xCtb, st->yCtb = yCtb;
    put(st->cc, states);
    st->cc.rate = Cost();
    Handle h{ st };
    h(coding_quadtree(xCtb, yCtb, st->ctbLog2, 0));
    take(st->cc, states);
    return st->cc.rate.value;
}
