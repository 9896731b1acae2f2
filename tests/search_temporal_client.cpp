// The per-call client once more (search_client.cpp, whole), with one entry point beside it: a picture's searches in dependency order WITH a table of temporal
// candidates (picture_order.hpp: walkPictureSequential's `temporal`) -- the expected values of havoc_mi355x_search_picture_uni after havoc_mi355x_search_temporal.
// Built into libraries of its own name for the `oracle` and `ref` back ends (tests/search_temporal_tools.py).
#include "search_client.cpp"

using namespace havoc_search;

extern "C" {

// temporal = TemporalCand[2 * n] (index 2 * p + list) or nullptr (the walk without a table).  report (optional) = int32 [2 * n][10], per derivation made from the
// field as the walk had it at that moment: 0 = the slot a candidate would take (0, 1; -1: none, the list has two different spatial predictors), found by deriving
// with two different sentinel candidates and looking where the results differ -- not by restating the rule; 1 = reserved; 2..5 = the pair derived without a
// candidate (x0, y0, x1, y1); 6..9 = the pair the walk's search ran with.
int client_picture_uni_temporal(int S, const void *src, intptr_t ss, const void *ref0, const void *ref1, intptr_t rs, const havoc_search_params *p,
                                const havoc_picture_pu *pus, const int32_t *ctu_first, int ctus_x, int ctus_y, const int64_t *mvp_rate, havoc_search_result *out,
                                int16_t *field_out, havoc_search_result *out_bi, const TemporalCand *temporal, int32_t *report)
{
    if (!g_open) return -1;
    const SearchParams sp = paramsOf(*p);
    const Cost rate[2] = {mvp_rate[0], mvp_rate[1]};
    MotionField field;
    auto run = [&](auto sampleTag) {
        typedef decltype(sampleTag) Sample;
        const Sample *refs[2] = {(const Sample *)ref0, (const Sample *)ref1};
        auto get = [&](int list, int x, int y, Mv *v) { return field.get(list, x, y, v); };
        auto search = [&](int pi, int list, const PuContext &pu) {
            if (report)
            {
                int32_t *r = report + 10 * (2 * pi + list);
                Mv none[2], a[2], b[2];
                const TemporalCand sentinelA = {{30001, -30002}, 1, 2}, sentinelB = {{-30003, 30004}, 1, 2};
                derivePredictors(pus[pi], list, sp.ctbSize, sp.picWidth, sp.picHeight, get, none);
                derivePredictors(pus[pi], list, sp.ctbSize, sp.picWidth, sp.picHeight, get, a, &sentinelA);
                derivePredictors(pus[pi], list, sp.ctbSize, sp.picWidth, sp.picHeight, get, b, &sentinelB);
                r[0] = a[0] != b[0] ? 0 : (a[1] != b[1] ? 1 : -1);
                r[1] = 0;
                r[2] = none[0].x; r[3] = none[0].y; r[4] = none[1].x; r[5] = none[1].y;
                r[6] = pu.mvp[0].x; r[7] = pu.mvp[0].y; r[8] = pu.mvp[1].x; r[9] = pu.mvp[1].y;
            }
            TableView<Sample> view(tables<Sample>(), (const Sample *)src + intptr_t(pu.y0) * ss + pu.x0, ss, Plane<Sample>{refs[list], rs}, pu.x0, pu.y0, pu.w, pu.h,
                                   sp.bitDepth);
            MotionSearch<TableView<Sample>> ms(sp, pu, view);
            return ms.run();
        };
        auto bi = [&](int pi, int list, const PuContext &pu, Mv other, Mv start) {
            (void)pi;
            HAVOC_ALIGN(32, Sample, ideal[64 * 64]);
            const LimitFullPelMv limit(pu, sp);
            makeIdealPredictor<Sample>(tables<Sample>(), ideal, (const Sample *)src + intptr_t(pu.y0) * ss + pu.x0, ss, Plane<Sample>{refs[1 - list], rs}, other, limit,
                                       pu.x0, pu.y0, pu.w, pu.h, sp.bitDepth);
            TableView<Sample> view(tables<Sample>(), ideal, 64, Plane<Sample>{refs[list], rs}, pu.x0, pu.y0, pu.w, pu.h, sp.bitDepth);
            return searchMotionBi(sp, pu, view, start);
        };
        walkPictureSequential(sp, pus, ctu_first, ctus_x, ctus_y, rate, search, out, field, bi, out_bi, temporal);
    };
    if (S == 1) run(uint8_t(0));
    else run(uint16_t(0));
    if (field_out)
        for (int l = 0; l < 2; ++l)
            for (size_t c = 0; c < size_t(field.cw) * field.ch; ++c)
            {
                const Mv v = MotionField::unpack(field.mv[l][c]);
                field_out[(size_t(l) * field.cw * field.ch + c) * 2 + 0] = field.valid[l][c] ? v.x : 0;
                field_out[(size_t(l) * field.cw * field.ch + c) * 2 + 1] = field.valid[l][c] ? v.y : 0;
            }
    return 0;
}

} // extern "C"
