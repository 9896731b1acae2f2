// TEST INFRASTRUCTURE ONLY.  turingcodec_amd/search/merge_list.hpp on the host: (a) deriveMergeCandidateList beside tests/merge.hpp's deriveMergeCandidates on the
// same rows -- both headers in this one translation unit --, (b) cqtMergeList, the host form of havoc_mi355x_cqt_merge_lists, for tests/merge_list_tools.py to hold its
// python restatement (and through it the device) against.  Compiled at test time into a temporary directory (-I turingcodec_amd/search: tests/merge.hpp includes
// "decision.hpp").  With -DMERGE_LIST_MAIN a stand-alone program over inputs it makes itself: what a host sanitizer build runs.
#include "../turingcodec_amd/search/merge_list.hpp"
#include "merge.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace havoc_search;
namespace ml = havoc_search::merge_list;

static_assert(sizeof(ml::CqtMergeParams) == 48 && sizeof(ml::CqtMergeRecord) == 64 && sizeof(TemporalCand) == 8 && sizeof(havoc_picture_pu) == 32, "the records merge_list_tools.py passes");

template <class Cand>
static Cand unpackCand(const int32_t *q)
{
    Cand c;
    c.predFlag[0] = q[0] != 0; c.predFlag[1] = q[1] != 0;
    c.refIdx[0] = q[2]; c.refIdx[1] = q[3];
    c.mv[0] = Mv(int16_t(q[4]), int16_t(q[5])); c.mv[1] = Mv(int16_t(q[6]), int16_t(q[7]));
    return c;
}

// a list as tests/search_client.cpp: client_merge writes it: int32 [5][8], a list the candidate does not use as zeros, places beyond maxCand as zeros
template <class Cand>
static void packList(const Cand *list, int maxCand, int32_t *o)
{
    std::memset(o, 0, 40 * sizeof(int32_t));
    for (int k = 0; k < maxCand; ++k)
    {
        const Cand &c = list[k];
        int32_t *q = o + 8 * k;
        q[0] = c.predFlag[0]; q[1] = c.predFlag[1];
        q[2] = c.predFlag[0] ? c.refIdx[0] : 0; q[3] = c.predFlag[1] ? c.refIdx[1] : 0;
        q[4] = c.predFlag[0] ? c.mv[0].x : 0; q[5] = c.predFlag[0] ? c.mv[0].y : 0; q[6] = c.predFlag[1] ? c.mv[1].x : 0; q[7] = c.predFlag[1] ? c.mv[1].y : 0;
    }
}

extern "C" {

// rows: int32 [n][64], client_merge's layout (Log2ParMrgLevel 2: the unit is its own).  outNew / outOld: int32 [n][40], the list by merge_list.hpp / by tests/merge.hpp;
// ret: int32 [n][2], the two return values
void merge_list_rows(const int32_t *rows, int n, int32_t *outNew, int32_t *outOld, int32_t *ret)
{
    for (int i = 0; i < n; ++i)
    {
        const int32_t *r = rows + 64 * i;
        const int maxCand = r[6] < 5 ? r[6] : 5;
        {
            ml::MergeCand nb[5], list[5];
            for (int k = 0; k < 5; ++k) nb[k] = unpackCand<ml::MergeCand>(r + 8 + 8 * k);
            const ml::PocTables poc = {r + 56, r + 60};
            ret[2 * i] = ml::deriveMergeCandidateList(nb, r[0], r[1], r[2], r[1], r[2], r[7] != 0, unpackCand<ml::MergeCand>(r + 48), r[3] != 0, r[4], r[5], poc, maxCand, list);
            packList(list, maxCand, outNew + 40 * i);
        }
        {
            MergeCandidate nb[5], list[5];
            for (int k = 0; k < 5; ++k) nb[k] = unpackCand<MergeCandidate>(r + 8 + 8 * k);
            ret[2 * i + 1] = deriveMergeCandidates(nb, r[0], r[1], r[2], r[1], r[2], r[7] != 0, unpackCand<MergeCandidate>(r + 48), r[3] != 0, r[4], r[5], r + 56, r + 60, maxCand, list);
            packList(list, maxCand, outOld + 40 * i);
        }
    }
}

// havoc_mi355x_cqt_merge_lists on the host: cqtMergeList per searched unit.  temporal may be null
void cqt_merge_lists_host(const void *params, const void *cells, const void *pus, int n, const void *temporal, void *out)
{
    const ml::CqtMergeParams &P = *static_cast<const ml::CqtMergeParams *>(params);
    const havoc_picture_pu *q = static_cast<const havoc_picture_pu *>(pus);
    ml::CqtMergeRecord *o = static_cast<ml::CqtMergeRecord *>(out);
    for (int p = 0; p < n; ++p)
        o[p] = ml::cqtMergeList(P, static_cast<const unsigned long long *>(cells), static_cast<const unsigned long long *>(temporal), p, q[p].x0, q[p].y0, q[p].w, q[p].h);
}

} // extern "C"

#ifdef MERGE_LIST_MAIN
// inputs of its own making (a 64-bit LCG): random rows through both headers, then a random committed map -- every CTU one 64x64 unit or sixty-four 8x8 units, some
// CTUs undecided, the tables sized EXACTLY so that a read beside them is a sanitizer's finding -- through cqtMergeList with and without temporal records
static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) { state = state * 6364136223846793005ull + 1442695040888963407ull; return uint32_t(state >> 33) % n; }

int main()
{
    const int n = 50000;
    std::vector<int32_t> rows(64 * size_t(n)), a(40 * size_t(n)), b(40 * size_t(n)), ret(2 * size_t(n));
    for (int i = 0; i < n; ++i)
    {
        int32_t *r = &rows[64 * size_t(i)];
        const int32_t head[8] = {int32_t(rnd(2)), 8 << rnd(3), 8 << rnd(3), int32_t(rnd(4) != 0), 1 + int32_t(rnd(4)), 1 + int32_t(rnd(4)), 1 + int32_t(rnd(5)), int32_t(rnd(2))};
        std::memcpy(r, head, sizeof head);
        for (int k = 0; k < 6; ++k)
        {
            int32_t *q = r + 8 + 8 * k;
            const uint32_t kind = rnd(4);
            q[0] = kind == 1 || kind == 3; q[1] = kind == 2 || kind == 3;
            q[2] = int32_t(rnd(4)); q[3] = int32_t(rnd(4));
            for (int j = 4; j < 8; ++j) q[j] = rnd(8) ? int32_t(rnd(3)) - 1 : (rnd(2) ? 32767 : -32768);
        }
        for (int j = 56; j < 64; ++j) r[j] = int32_t(rnd(3));
    }
    merge_list_rows(rows.data(), n, a.data(), b.data(), ret.data());
    int differ = 0;
    for (int i = 0; i < n; ++i)
        differ += std::memcmp(&a[40 * size_t(i)], &b[40 * size_t(i)], 160) != 0 || ret[2 * size_t(i)] != ret[2 * size_t(i) + 1];

    int lists = 0, matched = 0;
    for (int round = 0; round < 40; ++round)
    {
        const int W = 64 * (1 + int(rnd(3))) + 8 * int(rnd(8)), H = 64 * (1 + int(rnd(2))) + 8 * int(rnd(8)), cw = W / 8, ch = H / 8;
        std::vector<unsigned long long> cells(3 * size_t(cw) * ch);
        std::vector<havoc_picture_pu> pus;
        for (int y = 0; y < H; y += 64)
            for (int x = 0; x < W; x += 64)
            {
                const uint32_t kind = (x + 64 > W || y + 64 > H) ? 1 + rnd(2) : rnd(3);       // 0: one 64x64 unit, 1: 8x8 units, 2: undecided
                const int first = int(pus.size());
                if (kind == 0) pus.push_back(havoc_picture_pu{x, y, 64, 64, 6, 0, 1, 0});
                for (int cy = y / 8; cy < ch && cy < y / 8 + 8; ++cy)
                    for (int cx = x / 8; cx < cw && cx < x / 8 + 8; ++cx)
                    {
                        unsigned long long *c = &cells[3 * (size_t(cy) * cw + cx)];
                        if (kind == 1) pus.push_back(havoc_picture_pu{8 * cx, 8 * cy, 8, 8, 3, 3, 1, 0});
                        const int unit = kind == 0 ? first : int(pus.size()) - 1;
                        const unsigned long long mv = kind == 0 ? 0x0001000200030004ull : ((unsigned long long)rnd(3) | (unsigned long long)rnd(3) << 16 | (unsigned long long)rnd(3) << 32 | (unsigned long long)rnd(3) << 48);
                        c[0] = kind == 2 ? ~0ull : (unsigned long long)uint32_t(unit);
                        c[1] = kind == 2 ? ~0ull : mv;
                        c[2] = kind == 2 ? ~0ull : (unsigned long long)(kind == 0 ? 6 : 3) | (unsigned long long)rnd(3) << 16;
                    }
            }
        pus.push_back(havoc_picture_pu{W, 0, 8, 8, 3, 3, 1, 0});        // not inside the picture
        pus.push_back(havoc_picture_pu{0, 0, 16, 8, 4, 2, 0, 0});       // not square
        std::vector<TemporalCand> temporal(2 * pus.size());
        for (TemporalCand &t : temporal)
        {
            t.available = int16_t(rnd(2));
            t.mv[0] = t.available ? int16_t(rnd(3)) : int16_t(0);
            t.mv[1] = t.available ? int16_t(rnd(3)) : int16_t(0);
            t.source = t.available ? 2 : 0;
        }
        std::vector<ml::CqtMergeRecord> out(pus.size());
        for (int withTemporal = 0; withTemporal < 2; ++withTemporal)
        {
            const ml::CqtMergeParams P = {W, H, 6, 3, 1 + int32_t(rnd(5)), {0, int32_t(rnd(2)) * 8}, {0, 0, 0, 0, 0}};
            cqt_merge_lists_host(&P, cells.data(), pus.data(), int(pus.size()), withTemporal ? temporal.data() : nullptr, out.data());
            for (const ml::CqtMergeRecord &r : out)
            {
                lists += (r.w[7] >> 32 & 255) != 0;
                matched += (r.w[7] >> 48 & 255) != 255;
            }
        }
    }
    std::printf("rows %d differ %d lists %d matched %d\n", n, differ, lists, matched);
    return differ != 0 || lists == 0 || matched == 0;
}
#endif
