// nn2_depth_core.hpp -- the depth-limited reads x candidates search (get_nearest_neighbors_2set with neighbor_search_depth smaller
// than the number of candidates) as lane-level routines: one lane per read, shared by the kernels of nn2_depth.hpp and by the CPU
// emulator of tests/emul (g++, also under UBSan).
//
// The reference loop of one read i on the length-sorted merged list, best = len(i):
//     iteration j = 1, 2, ...: both stop tests (array end, |len_i - len_{i-+j}| > best; sticky, on every neighbour, target or not),
//     then i-j is aligned with k = best if its side is not stopped and it is a target, then i+j likewise (its stop flag dates from
//     before the down alignment of the same j); 0 <= d < best resets the row, d == best appends; break on both sides stopped, else
//     on processed >= depth (tested at the end of the iteration: depth + 1 alignments may be spent, depth = 0 is one iteration).
// The lengths ascend, so a side is stopped at iteration j exactly when the neighbour AT j differs by more than the best of that
// moment: a target p below i is aligned iff len_i - len_p <= best at the start of its iteration (above: len_p - len_i).  The
// iterations that matter ("events") are therefore the merge of the targets below and above i by |p - i|, down first on ties, and
// the loop's j is replaced by two cursors: targets consumed below (a) and above (b).
//
// Rounds (DESIGN.md "depth-limited 2-set search"): nn2_speculate walks whole events with best FROZEN and lists the targets it would
// align; the caller computes their distances with threshold k = frozen best (exact if <= k, else -1); nn2_replay runs the reference
// rule over the same events with the live best.  best only falls, so the live visits are a subsequence of the listed ones.
#pragma once
#include "band_core.hpp"

namespace isocon {

static constexpr uint32_t NN2_NONE = 0xffffffffu;
static constexpr uint32_t NN2_STOP_DOWN = 1u, NN2_STOP_UP = 2u, NN2_DONE = 4u, NN2_ERROR = 8u;
static constexpr uint32_t NN2_B_MAX = 32;          // most targets a round lists per read before it ends (+ 1: an event can hold two)

// the merged list: lengths of all entries, the ascending positions of the targets, the depth limit (clamped to 2^32 - 1)
struct NN2Set {
    const int32_t *lens;
    const uint32_t *tpos;
    uint32_t nt;
    uint32_t depth;
};

// one read: targets consumed below / above it, the live threshold, alignments spent, NN2_* flags
struct NN2Lane {
    uint32_t a, b;
    int32_t best;
    uint32_t processed;
    uint32_t flags;
};

// The next event of read i (ti = number of targets below i): its offset j and the targets at i - j / i + j (NN2_NONE: none, or the
// side is stopped).  false: no target is left on a side that is still open.
ISO_HD bool nn2_next(const NN2Set &S, uint32_t i, uint32_t ti, uint32_t a, uint32_t b, uint32_t flags, uint32_t &j, uint32_t &pd, uint32_t &pu)
{
    pd = (!(flags & NN2_STOP_DOWN) && a < ti) ? S.tpos[ti - 1u - a] : NN2_NONE;
    pu = (!(flags & NN2_STOP_UP) && b < S.nt - ti) ? S.tpos[ti + b] : NN2_NONE;
    const uint32_t jd = pd != NN2_NONE ? i - pd : NN2_NONE, ju = pu != NN2_NONE ? pu - i : NN2_NONE;
    j = jd < ju ? jd : ju;
    if (j == NN2_NONE) return false;
    if (jd != j) pd = NN2_NONE;
    if (ju != j) pu = NN2_NONE;
    return true;
}

// Step 1.  Walks events from the lane's state with best frozen and calls emit(target) for every alignment the reference could make,
// in its order; ends after the first event at which `want` targets are out (want = min(B, alignments the depth rule still allows)),
// at which both sides are stopped, or when the targets run out.  Returns the number emitted (<= B + 1); j_end = the last event walked
// (0: none).
template <class Emit>
ISO_HD uint32_t nn2_speculate(const NN2Set &S, uint32_t i, uint32_t ti, const NN2Lane &L, uint32_t B, uint32_t &j_end, Emit emit)
{
    j_end = 0;
    if (L.flags & NN2_DONE) return 0;
    const int32_t li = S.lens[i], frozen = L.best;
    uint32_t a = L.a, b = L.b, flags = L.flags, out = 0;
    const uint32_t left = S.depth > L.processed ? S.depth - L.processed : 1u;
    const uint32_t want = B < left ? B : left;
    for (;;) {
        uint32_t j, pd, pu;
        if (!nn2_next(S, i, ti, a, b, flags, j, pd, pu)) break;
        if (S.depth == 0 && j > 1) break;          // (the only iteration of depth 0 held no target)
        j_end = j;
        if (pd != NN2_NONE) {
            if (li - S.lens[pd] > frozen) flags |= NN2_STOP_DOWN;
            else { emit(pd); ++out; }
            ++a;
        }
        if (pu != NN2_NONE) {
            if (S.lens[pu] - li > frozen) flags |= NN2_STOP_UP;
            else { emit(pu); ++out; }
            ++b;
        }
        if ((flags & (NN2_STOP_DOWN | NN2_STOP_UP)) == (NN2_STOP_DOWN | NN2_STOP_UP) || out >= want) break;
    }
    return out;
}

// Step 3.  The reference rule over the events up to j_end with the live state.  spec_t / spec_d: the n_spec targets step 1 listed
// for this read and their distances (exact if <= the frozen best, else -1); a distance above the live best counts as -1, which is
// what an alignment with k = best would have returned.  hit(target, d) is called for every d <= best of its moment, in the
// reference's visiting order: the read's row is the hits with d == final best, in that order.
template <class Hit>
ISO_HD void nn2_replay(const NN2Set &S, uint32_t i, uint32_t ti, NN2Lane &L, uint32_t j_end, const uint32_t *spec_t, const int32_t *spec_d,
                       uint32_t n_spec, Hit hit)
{
    if (L.flags & NN2_DONE) return;
    const int32_t li = S.lens[i];
    uint32_t s = 0;
    auto visit = [&](uint32_t p) {
        while (s < n_spec && spec_t[s] != p) ++s;          // (listed under a frozen best that a side's live stop has since overtaken)
        if (s == n_spec) { L.flags |= NN2_ERROR; return; }
        const int32_t d = spec_d[s++];
        ++L.processed;
        if (d < 0 || d > L.best) return;
        if (d < L.best) L.best = d;
        hit(p, d);
    };
    for (;;) {
        uint32_t j, pd, pu;
        if (!nn2_next(S, i, ti, L.a, L.b, L.flags, j, pd, pu)) { L.flags |= NN2_DONE; break; }
        if (S.depth == 0 && j > 1) { L.flags |= NN2_DONE; break; }
        if (j > j_end) break;
        const int32_t best0 = L.best;          // both stop tests precede the alignments of the iteration
        const bool stop_d = pd != NN2_NONE && li - S.lens[pd] > best0, stop_u = pu != NN2_NONE && S.lens[pu] - li > best0;
        if (pd != NN2_NONE) {
            if (stop_d) L.flags |= NN2_STOP_DOWN;
            else visit(pd);
            ++L.a;
        }
        if (pu != NN2_NONE) {
            if (stop_u) L.flags |= NN2_STOP_UP;
            else visit(pu);
            ++L.b;
        }
        if ((L.flags & (NN2_STOP_DOWN | NN2_STOP_UP)) == (NN2_STOP_DOWN | NN2_STOP_UP) || L.processed >= S.depth || (L.flags & NN2_ERROR)) {
            L.flags |= NN2_DONE;
            break;
        }
    }
}

// Between steps 1 and 2 the block bound of nn_filter.hpp looks at the listed pairs (k_nn2_block_reject, nn2_depth.hpp): a pair whose
// greedy count of disjoint 8-grams of the target that occur nowhere in the read exceeds k has a distance above k, i.e. the -1 its slot
// already holds.  A wave takes a TASK: up to NN2_TASK_PAIRS consecutive pairs of one read's run in the pair arrays.
static constexpr uint32_t NN2_TASK_PAIRS = 64;
static constexpr int32_t NN2_REJECTED = -2;          // pk_lanes of a pair the block bound has decided (-1: an entry outside the planes' map)
static constexpr int NN2_PROBE_STRIDE = 2;           // bases between two probes of the test (2 or 4; profiles/nn2set_depth.txt)

struct NN2Task { uint32_t read, count; unsigned long long begin; };

// Whether the test looks at a pair: k = its threshold for the 64-row kernel (negative: not for the bit-vector kernels), len_t = the
// target's length.  A target holds at most len_t / 8 disjoint 8-grams, so with k >= len_t / 8 the count cannot exceed k.
ISO_HD bool nn2_tested(int32_t k, int32_t len_t) { return k >= 0 && k < len_t / 8; }

// Cuts the run [begin, begin + count) of one read's pairs into tasks: emit(first, pairs) for ranges of at most NN2_TASK_PAIRS pairs
// that start and end with a tested pair and together hold every tested pair once (tested(p): pair p is one); untested pairs in
// between ride along as idle lanes.  A run without a tested pair makes no task.  Returns the number of tasks.
template <class Tested, class Emit>
ISO_HD uint32_t nn2_cut_tasks(unsigned long long begin, unsigned long long count, Tested tested, Emit emit)
{
    const unsigned long long end = begin + count;
    uint32_t n_tasks = 0;
    unsigned long long p = begin;
    for (;;) {
        while (p < end && !tested(p)) ++p;
        if (p >= end) break;
        const unsigned long long stop = end - p > NN2_TASK_PAIRS ? p + NN2_TASK_PAIRS : end;
        unsigned long long last = p;
        for (unsigned long long t = p + 1; t < stop; ++t)
            if (tested(t)) last = t;
        emit(p, (uint32_t)(last - p + 1));
        ++n_tasks;
        p = last + 1;
    }
    return n_tasks;
}

// A whole pair list whose runs of equal read[] are the reads' runs (the test entry isocon_nn2_block_reject; the search's listing kernel
// knows its run and calls nn2_cut_tasks itself): emit(read, first, pairs) per task.  Returns the number of tasks.
template <class Tested, class Emit>
inline unsigned long long nn2_cut_list(const uint32_t *read, unsigned long long n_pairs, Tested tested, Emit emit)
{
    unsigned long long n_tasks = 0;
    for (unsigned long long b = 0, e; b < n_pairs; b = e) {
        for (e = b + 1; e < n_pairs && read[e] == read[b]; ++e) {}
        const uint32_t x = read[b];
        n_tasks += nn2_cut_tasks(b, e - b, tested, [&](unsigned long long first, uint32_t pairs) { emit(x, first, pairs); });
    }
    return n_tasks;
}

}  // namespace isocon
