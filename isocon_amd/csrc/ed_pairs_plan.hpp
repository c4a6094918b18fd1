// ed_pairs_plan.hpp -- host-side routing of an explicit pair list through the distance stages (ed_pairs_impl in isocon_hip.hip: isocon_ed_pairs
// and the fallback of the nearest-neighbour and path entry points): which side of the pairs is the shared one, the order, which pairs go one
// per lane and which in 64-lane tiles of one shared sequence, the re-tiling of the lanes a tile could not certify, the escalation over
// 64, 128, 256 and 512 band rows and the hand-over to the un-banded stage.  The stages themselves sit behind a backend of three calls
//     int lanes(a, b, k, out)            one pair per lane (ed_lanes.hpp), out[i] = distance if <= k[i], else -1
//     int tiles(W, ts, ids, ks, out)     64 * W band rows (ed_band.hpp): tile t aligns sequence ts[t] with ids[64 t .. 64 t + 63] (0xffffffff: empty
//                                        lane, k = -1); out = distance, -1 (beyond ks) or -2 (this tile's window could not certify ks for the lane)
//     int full(a, b, k, out)             the un-banded stage (ed_full.hpp), k < 0: unbounded; a status other than ISOCON_OK ends the plan
// Plain C++ (no HIP), like the byte-range copy of the gathered upload at the end: tests/emul/ed_pairs_plan_emul.cpp drives both (the CPU emulators
// of the stages behind the backend), with g++ -fsanitize=address,undefined.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/isocon_hip.h"

namespace {

// The threshold a pair with its own k (k < 0: unbounded) gets in a stage that certifies distances up to kcap.
inline int32_t ed_stage_threshold(int32_t k, int32_t kcap) { return k < 0 ? kcap : std::min(k, kcap); }

// What a stage's answer r settles: the distance, else "beyond k" (-1) if the pair's own k is within the stage's cap.  false: on to the next stage.
inline bool ed_stage_settles(int32_t r, int32_t k, int32_t kcap, int32_t *out)
{
    if (r >= 0) { *out = r; return true; }
    if (k >= 0 && k <= kcap) { *out = -1; return true; }
    return false;
}

// Exact bounded / unbounded distances of the pairs `pending` (indices into a, b, k; k == nullptr: all unbounded) into out_ed.  lens: the
// sequences' lengths (n of them; a and b are in range).  The shared side is chosen over all n_pairs.  min_group: the pairs of a shared
// sequence with fewer partners than this go one per lane instead of into a tile.  *full_pairs: how many reached the un-banded stage.
template <class Backend>
inline int ed_pairs_plan(const int32_t *lens, uint32_t n, const uint32_t *a, const uint32_t *b, const int32_t *k, uint64_t n_pairs, std::vector<uint64_t> pending,
                         size_t min_group, Backend &stages, int32_t *out_ed, uint64_t *full_pairs, std::string &error)
{
    // which side is shared more often?  (edit distance is symmetric)
    std::vector<uint8_t> seen_a(n, 0), seen_b(n, 0);
    size_t da = 0, db = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        if (!seen_a[a[p]]) { seen_a[a[p]] = 1; ++da; }
        if (!seen_b[b[p]]) { seen_b[b[p]] = 1; ++db; }
    }
    const bool swap_roles = db < da;
    auto sh = [&](uint64_t p) { return swap_roles ? b[p] : a[p]; };
    auto ln = [&](uint64_t p) { return swap_roles ? a[p] : b[p]; };
    auto kreq = [&](uint64_t p) { return k ? k[p] : -1; };
    int rc;
    for (int W = 1; W <= 8 && !pending.empty(); W *= 2) {
        const int32_t kcap = 64 * W - 1;
        std::sort(pending.begin(), pending.end(), [&](uint64_t x, uint64_t y) {
            if (sh(x) != sh(y)) return sh(x) < sh(y);
            const int32_t lx = lens[ln(x)], ly = lens[ln(y)];
            if (lx != ly) return lx < ly;
            return x < y;
        });
        std::vector<uint64_t> todo = pending, next;
        if (W == 1) {
            // Pairs that share their sequence with fewer than min_group others would leave most lanes of a tile empty: one pair per
            // lane instead (ed_lanes.hpp; ~1.7x the column cost, every lane busy).
            std::vector<uint64_t> lanes_p, tiles_p;
            for (size_t i = 0; i < todo.size();) {
                size_t j = i;
                while (j < todo.size() && sh(todo[j]) == sh(todo[i])) ++j;
                std::vector<uint64_t> &dst = (j - i) < min_group ? lanes_p : tiles_p;
                dst.insert(dst.end(), todo.begin() + i, todo.begin() + j);
                i = j;
            }
            if (!lanes_p.empty()) {
                const size_t np = lanes_p.size();
                std::vector<uint32_t> la(np), lb(np);
                std::vector<int32_t> lk(np), res;
                for (size_t i = 0; i < np; ++i) { la[i] = a[lanes_p[i]]; lb[i] = b[lanes_p[i]]; lk[i] = ed_stage_threshold(kreq(lanes_p[i]), kcap); }
                if ((rc = stages.lanes(la, lb, lk, res))) return rc;
                for (size_t i = 0; i < np; ++i)
                    if (!ed_stage_settles(res[i], kreq(lanes_p[i]), kcap, &out_ed[lanes_p[i]])) next.push_back(lanes_p[i]);
            }
            todo.swap(tiles_p);
        }
        for (int round = 0; round < 2 && !todo.empty(); ++round) {
            // round 0: tiles of up to 64 lanes per shared sequence; round 1: one lane per tile for pairs whose
            // tile could not certify the threshold (heterogeneous length differences)
            std::vector<uint32_t> ts, ids;
            std::vector<int32_t> ks, res;
            std::vector<uint64_t> slot_pair, retry;          // slot_pair: the pair in every lane slot, ~0 for padding
            const size_t lanes_per_tile = round == 0 ? 64 : 1;
            for (size_t i = 0; i < todo.size();) {
                size_t j = i;
                const uint32_t s0 = sh(todo[i]);
                while (j < todo.size() && j - i < lanes_per_tile && sh(todo[j]) == s0) ++j;
                ts.push_back(s0);
                for (size_t l = 0; l < 64; ++l) {
                    const bool lane = i + l < j;
                    const uint64_t p = lane ? todo[i + l] : ~(uint64_t)0;
                    ids.push_back(lane ? ln(p) : 0xffffffffu);
                    ks.push_back(lane ? ed_stage_threshold(kreq(p), kcap) : -1);
                    slot_pair.push_back(p);
                }
                i = j;
            }
            if ((rc = stages.tiles(W, ts, ids, ks, res))) return rc;
            for (size_t s = 0; s < slot_pair.size(); ++s) {
                const uint64_t p = slot_pair[s];
                if (p == ~(uint64_t)0) continue;
                if (res[s] == -2) retry.push_back(p);
                else if (!ed_stage_settles(res[s], kreq(p), kcap, &out_ed[p])) next.push_back(p);
            }
            todo.swap(retry);
        }
        if (!todo.empty()) { error = "internal: single-lane tile undetermined"; return ISOCON_E_HIP; }
        pending.swap(next);
    }
    if (full_pairs) *full_pairs = pending.size();
    if (!pending.empty()) {
        std::vector<uint32_t> fa, fb;
        std::vector<int32_t> fk, res;
        for (uint64_t p : pending) { fa.push_back(a[p]); fb.push_back(b[p]); fk.push_back(kreq(p)); }
        if ((rc = stages.full(fa, fb, fk, res))) return rc;
        for (size_t i = 0; i < pending.size(); ++i) out_ed[pending[i]] = res[i];
    }
    return ISOCON_OK;
}

// The gathered upload of a store's creation (upload_gathered in isocon_hip.hip): the sequences lie scattered in host memory and go up as
// their concatenation.  bytes [b0, b1) of the concatenation of seq_ptrs[0 .. n) -> dst; offsets[0 .. n]: the sequences' prefix sums.
inline void gather_bytes(char *dst, const uint8_t *const *seq_ptrs, const uint64_t *offsets, uint32_t n, uint64_t b0, uint64_t b1)
{
    const uint64_t base = offsets[0];
    uint32_t i = (uint32_t)(std::upper_bound(offsets, offsets + n + 1, base + b0) - offsets) - 1;
    uint64_t in_seq = base + b0 - offsets[i];
    while (b0 < b1 && i < n) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        const size_t take = (size_t)std::min<uint64_t>(len - in_seq, b1 - b0);
        if (take) memcpy(dst, seq_ptrs[i] + in_seq, take);
        dst += take; b0 += take; in_seq += take;
        if (in_seq == len) { ++i; in_seq = 0; }
    }
}

}  // namespace
