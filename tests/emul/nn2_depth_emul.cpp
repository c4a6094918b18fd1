// CPU driver of isocon_amd/csrc/nn2_depth_core.hpp (tests/test_nn2set_depth_core.py): the two lane routines of the depth-limited 2-set
// search, one call per round and step over all reads, the way the kernels of nn2_depth.hpp call them.  The distances between the two
// steps come from the caller (the oracle).
#include <cstdint>

#include "../../isocon_amd/csrc/nn2_depth_core.hpp"

using namespace isocon;

extern "C" {

// Step 1 for every read r (entry qidx[r], tiq[r] targets below it).  Pairs of read r: slots pbase[r] .. pbase[r] + pcnt[r] of pa / pb / pk
// (read, target, frozen best).  Returns the number of pairs, or -1 if they do not fit cap.
int64_t nn2_emul_speculate(const int32_t *lens, const uint32_t *tpos, uint32_t nt, uint32_t depth, uint32_t B, uint32_t nq, const uint32_t *qidx,
                           const uint32_t *tiq, const NN2Lane *lanes, uint32_t *jend, uint32_t *pbase, uint32_t *pcnt, uint32_t *pa, uint32_t *pb,
                           int32_t *pk, uint64_t cap)
{
    const NN2Set S{lens, tpos, nt, depth};
    uint64_t total = 0;
    for (uint32_t r = 0; r < nq; ++r) {
        const uint32_t i = qidx[r];
        uint32_t je = 0;
        const uint32_t cnt = nn2_speculate(S, i, tiq[r], lanes[r], B, je, [](uint32_t) {});
        if (cnt > B + 1 || total + cnt > cap) return -1;
        uint64_t at = total;
        nn2_speculate(S, i, tiq[r], lanes[r], B, je, [&](uint32_t p) { pa[at] = i; pb[at] = p; pk[at] = lanes[r].best; ++at; });
        jend[r] = je;
        pbase[r] = (uint32_t)total;
        pcnt[r] = cnt;
        total += cnt;
    }
    return (int64_t)total;
}

// Step 3 for every read; hits are appended as (read, target, d).  Returns the number of reads that are not done, -1 on an internal
// error (a live visit that step 1 had not listed), -2 if the hits do not fit.
int64_t nn2_emul_replay(const int32_t *lens, const uint32_t *tpos, uint32_t nt, uint32_t depth, uint32_t nq, const uint32_t *qidx, const uint32_t *tiq,
                        NN2Lane *lanes, const uint32_t *jend, const uint32_t *pbase, const uint32_t *pcnt, const uint32_t *pb, const int32_t *pd,
                        int32_t *hits, uint64_t hits_cap, uint64_t *n_hits)
{
    const NN2Set S{lens, tpos, nt, depth};
    int64_t open = 0;
    bool full = false;
    for (uint32_t r = 0; r < nq; ++r) {
        const uint32_t i = qidx[r];
        nn2_replay(S, i, tiq[r], lanes[r], jend[r], pb + pbase[r], pd + pbase[r], pcnt[r], [&](uint32_t p, int32_t d) {
            if (*n_hits >= hits_cap) { full = true; return; }
            int32_t *h = hits + *n_hits * 3;
            h[0] = (int32_t)i; h[1] = (int32_t)p; h[2] = d;
            ++*n_hits;
        });
        if (lanes[r].flags & NN2_ERROR) return -1;
        if (!(lanes[r].flags & NN2_DONE)) ++open;
    }
    return full ? -2 : open;
}

}  // extern "C"
