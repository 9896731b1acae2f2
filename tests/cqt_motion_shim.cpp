// TEST INFRASTRUCTURE ONLY.  The reference's own collocated motion store: a real StateCollocatedMotion (turing/StateCollocatedMotion.h:51-122) over an empty decoded
// picture buffer, filled only through the reference's own fillRectangle (:75-90), once per committed coding unit in the order the caller gives, with a PuData that
// carries the unit's vectors and refIdxPlus1 / dpbIndexPlus1.  Compiled with oracle/Makefile's TURFLAGS into a temporary directory by tests/cqt_motion_tools.py;
// nothing of the reference is stored.
#include "turing/StateCollocatedMotion.h"
#include <cstdint>
#include <vector>

namespace {

// what the constructor reads of a decoded picture buffer's entries; the buffer here is empty, the loop body only has to compile
struct NoPicture
{
    int reference;
    int32_t operator[](PicOrderCntVal) const { return 0; }
};

}

// g: int32 [2] = width, height.  units: int32 [n][10] = x0, y0, size, predFlag0, predFlag1, mv0 x, y, mv1 x, y, reserved.  dpb0 / dpb1: the dpb indices of the
// pictures behind lists 0 and 1.  entries: int32 [rows * stride][8] = predFlag0, predFlag1, mv0 x, y, mv1 x, y, dpbIndex0, dpbIndex1 (-1: none); returns stride
extern "C" int cqt_motion_entries(const int32_t *g, const int32_t *units, int n, int dpb0, int dpb1, int32_t *entries)
{
    std::vector<const NoPicture *> dpb;
    StateCollocatedMotion store(g[0], g[1], dpb, 0);
    for (int i = 0; i < n; ++i)
    {
        const int32_t *u = units + 10 * i;
        PuData pu = PuData();
        for (int l = 0; l < 2; ++l)
            if (u[3 + l])
            {
                pu.refIdxPlus1[l] = 1;                                  // reference index 0
                pu.inter.dpbIndexPlus1[l] = int8_t((l ? dpb1 : dpb0) + 1);
                pu.mv(l)[0] = int16_t(u[5 + 2 * l]);
                pu.mv(l)[1] = int16_t(u[6 + 2 * l]);
            }
        store.fillRectangle(prediction_unit(u[0], u[1], u[2], u[2]), pu);
    }
    const int stride = int(store.stride), rows = int(store.entries.size()) / stride;
    for (int i = 0; i < rows * stride; ++i)
    {
        const PuData &e = store.entries[i];
        int32_t *o = entries + 8 * i;
        o[0] = e.predFlag(0); o[1] = e.predFlag(1);
        for (int l = 0; l < 2; ++l) o[2 + 2 * l] = e.mv(l)[0], o[3 + 2 * l] = e.mv(l)[1];
        o[6] = e.getDpbIndex(0); o[7] = e.getDpbIndex(1);
    }
    return stride;
}
