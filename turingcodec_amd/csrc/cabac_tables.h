// CABAC tables shared by the kernels that estimate rates: the bits of a bin from each context state, and the spec's state transitions.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace havoc_gpu {

namespace {

// turing/Write.h:413-422: estimated bits (Q15) for the more / less probable symbol from each CABAC state
__device__ const int32_t kEntropyBits[128] = {
    0x07b23, 0x085f9, 0x074a0, 0x08cbc, 0x06ee4, 0x09354, 0x067f4, 0x09c1b, 0x060b0, 0x0a62a, 0x05a9c, 0x0af5b, 0x0548d, 0x0b955, 0x04f56, 0x0c2a9,
    0x04a87, 0x0cbf7, 0x045d6, 0x0d5c3, 0x04144, 0x0e01b, 0x03d88, 0x0e937, 0x039e0, 0x0f2cd, 0x03663, 0x0fc9e, 0x03347, 0x10600, 0x03050, 0x10f95,
    0x02d4d, 0x11a02, 0x02ad3, 0x12333, 0x0286e, 0x12cad, 0x02604, 0x136df, 0x02425, 0x13f48, 0x021f4, 0x149c4, 0x0203e, 0x1527b, 0x01e4d, 0x15d00,
    0x01c99, 0x166de, 0x01b18, 0x17017, 0x019a5, 0x17988, 0x01841, 0x18327, 0x016df, 0x18d50, 0x015d9, 0x19547, 0x0147c, 0x1a083, 0x0138e, 0x1a8a3,
    0x01251, 0x1b418, 0x01166, 0x1bd27, 0x01068, 0x1c77b, 0x00f7f, 0x1d18e, 0x00eda, 0x1d91a, 0x00e19, 0x1e254, 0x00d4f, 0x1ec9a, 0x00c90, 0x1f6e0,
    0x00c01, 0x1fef8, 0x00b5f, 0x208b1, 0x00ab6, 0x21362, 0x00a15, 0x21e46, 0x00988, 0x2285d, 0x00934, 0x22ea8, 0x008a8, 0x239b2, 0x0081d, 0x24577,
    0x007c9, 0x24ce6, 0x00763, 0x25663, 0x00710, 0x25e8f, 0x006a0, 0x26a26, 0x00672, 0x26f23, 0x005e8, 0x27ef8, 0x005ba, 0x284b5, 0x0055e, 0x29057,
    0x0050c, 0x29bab, 0x004c1, 0x2a674, 0x004a7, 0x2aa5e, 0x0046f, 0x2b32f, 0x0041f, 0x2c0ad, 0x003e7, 0x2ca8d, 0x003ba, 0x2d323, 0x0010c, 0x3bfbb };

// H.265 Table 9-53 (transIdxLps): the probability state after a least probable symbol; after a most probable one it is
// min(pStateIdx + 1, 62) (63 stays 63), and an LPS in state 0 swaps valMps (9.3.4.3.2.2)
__device__ const uint8_t kTransIdxLps[64] = {
    0, 0, 1, 2, 2, 4, 4, 5, 6, 7, 8, 9, 9, 11, 11, 12, 13, 13, 15, 15, 16, 16, 18, 18, 19, 19, 21, 21, 22, 22, 23, 24,
    24, 25, 26, 26, 27, 27, 28, 29, 29, 30, 30, 30, 31, 32, 32, 33, 33, 33, 34, 34, 35, 35, 35, 36, 36, 36, 37, 37, 37, 38, 38, 63 };

// measureEncodeDecision (Write.h:476-492) as the context-updating EstimateRate uses it (Search<sao>::go, residual_coding): the Q15 bits of the bin from this
// state, as a Q16 Cost, then the state transition of H.265 9.3.4.3.2.2 (kTransIdxLps; an LPS in state 0 swaps the MPS).  Entry
// 2 state + bin of a walk's LDS table: the new state | the rate << 8 (a walk prices its dependent bins with one LDS read each)
__device__ __forceinline__ int bin_entry(int state, int bin)
{
    const int i = state ^ bin, p = state >> 1;
    int mps = state & 1, np;
    if (i & 1)
    {
        np = kTransIdxLps[p];
        if (p == 0) mps = bin;
    }
    else
        np = p < 62 ? p + 1 : p;
    return (np << 1 | mps) | kEntropyBits[i] << 9;
}

__device__ __forceinline__ long long ctx_bin(const int *table, int &state, int bin)
{
    const int e = table[2 * state + bin];
    state = e & 0xff;
    return (long long)(e >> 8);
}

} // namespace

} // namespace havoc_gpu
