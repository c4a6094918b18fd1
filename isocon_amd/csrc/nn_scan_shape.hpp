// nn_scan_shape.hpp -- launch shapes of the table kernels of the nearest-neighbour search (k_nn_scan_refill, k_nn_scan_lds, k_nn_scan_up in
// nn.hpp), derived from the longest sequence of the store: the one place that knows how much LDS a workgroup takes and how many waves
// it gets.  Plain C++: no HIP types, so that tests/emul/nn_scan_shape_main.cpp can compile it with g++ -fsanitize=undefined,address
// (tests/test_nn_scan_shape.py).
#pragma once
#include <cstddef>
#include <cstdint>

namespace isocon {

static constexpr int NN_RING = 96;                           // k_nn_scan_refill: queue entries per wave (8 B each)
static constexpr size_t NN_CU_LDS = (size_t)160 * 1024;      // LDS of a compute unit = the most one workgroup can have

// Dynamic LDS of k_nn_scan_refill for a band of `rows` rows (32: the HALF form, 64 W: the W-word form): four match-mask planes of
// (maxlen + 3 rows) dwords, rounded up to 32, and 2 rows + 32 dwords of ones for the virtual columns (layout: nn.hpp).
inline size_t nn_refill_lds(int32_t maxlen, int rows) { return ((size_t)4 * ((maxlen + 3 * rows + 31) & ~31) + 2 * rows + 32) * 4; }

// Static LDS of a workgroup of `waves` waves: the waves' queues and the workgroup's counter.
inline size_t nn_ring_bytes(int waves) { return (size_t)waves * NN_RING * 8 + 16; }

// Can one workgroup of `waves` waves hold the table of the longest sequence?
inline bool nn_refill_fits(int32_t maxlen, int rows, int waves) { return nn_refill_lds(maxlen, rows) + nn_ring_bytes(waves) <= NN_CU_LDS; }

// The 64-row kernel runs at all: in its largest form, 16 waves (the 32-row form needs less: whatever passes here may launch both).
inline bool nn_refill64_fits(int32_t maxlen) { return nn_refill_fits(maxlen, 64, 16); }

struct NNRefillShape {
    int waves;               // 4, 8 or 16: the NWAVES of the instantiation
    size_t lds;              // dynamic LDS of the launch
    bool raise_limit;        // more than the 64 KB a kernel gets unasked: hipFuncAttributeMaxDynamicSharedMemorySize first
};

// Waves per workgroup of a 64-row (half: 32-row) launch.  While three 8-wave workgroups fit a compute unit the caller's preference
// holds (4, anything else counts as 8); beyond that a table is alone on its compute unit and gets all 16 waves.
inline NNRefillShape nn_refill_shape(int32_t maxlen, int preferred_waves, bool half)
{
    const size_t lds = nn_refill_lds(maxlen, half ? 32 : 64);
    if (3 * (lds + nn_ring_bytes(8)) <= NN_CU_LDS) return NNRefillShape{preferred_waves == 4 ? 4 : 8, lds, false};
    return NNRefillShape{16, lds, true};
}

// Occupancy experiment (variant nn_lds_pad): the 8-wave 64-row launch with `pad` more bytes per workgroup (3 -> 2 -> 1 workgroups per CU).
inline NNRefillShape nn_refill_shape_padded(int32_t maxlen, int pad) { return NNRefillShape{8, nn_refill_lds(maxlen, 64) + (size_t)pad, true}; }

// The main pass without the refill kernel (tile-synchronous kernels on interleaved planes): the table is (maxlen + 192) entries of 16 B.
enum NNTileScan {
    NN_SCAN_LDS8,            // k_nn_scan_lds<8>: three 8-wave workgroups per CU
    NN_SCAN_LDS16,           // k_nn_scan_lds<16>: long reads, one 16-wave workgroup per table (raised limit)
    NN_SCAN_WINDOW           // k_nn_scan_up<1>: > 10 kb, scalar window, no table
};
inline size_t nn_tile_scan_lds(int32_t maxlen) { return (size_t)(maxlen + 192) * 16; }
inline NNTileScan nn_tile_scan(int32_t maxlen)
{
    const size_t lds = nn_tile_scan_lds(maxlen);
    return lds <= 53 * 1024 ? NN_SCAN_LDS8 : lds <= NN_CU_LDS ? NN_SCAN_LDS16 : NN_SCAN_WINDOW;
}

}  // namespace isocon
