/*
 * isocon_hip.h -- C ABI of libisocon_hip.so: the MI355X (gfx950) implementation of IsoCon's all-pairs alignment +
 * nearest-neighbour-graph hot path.
 *
 * The reference (ksahlin/IsoCon v0.3.3) is pure Python and has NO FFI for this path: its arithmetic is reached
 * through the Python bindings of two third-party libraries (edlib, parasail).  Each entry point below therefore
 * cites the reference *call site(s)* it replaces (paths relative to the reference root); the Python modules in
 * isocon_amd/ bind them with ctypes and re-create the reference's function signatures on top
 * (see INTEGRATION.md).
 *
 * Conventions: plain pointers and sizes only; the caller owns every buffer; every function returns an
 * isocon_status (0 = OK, negative = error) and never throws; all calls block until results are in host memory.
 * Alphabet.  Sequences are upper-case ACGT in all shipped data.  edlib compares whatever characters it is given
 * (modules/edlib_alignment_module.py:111, modules/nearest_neighbor_graph.py:105), so the distance and nearest-neighbour entry points
 * take ANY bytes, with the same results as a textbook edit distance over those bytes ('N' equals 'N', 'a' differs from 'A'):
 *   - a set over at most four distinct symbols (lower case, RNA ...) is packed in two bits per base under its own symbol map and runs
 *     through the same kernels as ACGT (distances, nearest neighbours, infix alignments);
 *   - a set with MORE than four distinct symbols (ACGT + N, mixed case) keeps its bytes on the device beside the 2-bit planes, which then
 *     hold class-merged IMAGES of the sequences (lower case folded onto upper case, other bytes onto one code: d(images) <= d).  The
 *     nearest-neighbour search finds its candidates on the images with the ordinary kernels; a candidate pair in which a sequence holds a
 *     symbol outside ACGT gets its exact distance from a byte-wise kernel (one wavefront per pair, much slower per pair than the bit-vector
 *     kernels -- isocon_nn_stats.pairs_bytes counts them); pairs of two ACGT sequences are not affected.  isocon_ed_pairs and the
 *     nearest-neighbour entry points serve such a set; isocon_hw_pairs and the q-gram bound test entry points return ISOCON_E_ALPHABET.
 * The alignment and consensus entry points need ACGT (the reference builds its parasail matrix on "ACGT",
 * modules/SW_alignment_module.py:65; what parasail does off that alphabet is not pinned): ISOCON_E_ALPHABET on any other set.
 */
#ifndef ISOCON_HIP_H
#define ISOCON_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    ISOCON_OK = 0,
    ISOCON_E_ARG = -1,        /* bad argument */
    ISOCON_E_ALPHABET = -2,   /* an entry point that needs ACGT (alignments, consensus) or 2-bit planes (infix, bound tests) on a set that is not such */
    ISOCON_E_HIP = -3,        /* HIP runtime error (isocon_last_error() has the text) */
    ISOCON_E_CAPACITY = -4,   /* caller buffer too small; required size written back */
    ISOCON_E_NODEVICE = -5,   /* no usable GPU */
    ISOCON_E_UNSUPPORTED = -6
} isocon_status;

typedef struct isocon_store isocon_store; /* opaque: packed sequence set resident in HBM */

/* Select the HIP device for subsequent calls of this process (one process per GPU). */
int isocon_init(int device_ordinal);
const char *isocon_strerror(int status);
const char *isocon_last_error(void);
int isocon_device_count(void);
/* Free the process-wide device scratch (trace buffers, hit lists ...) that calls keep for reuse. */
void isocon_release_scratch(void);

/*
 * Pack n sequences (ASCII, concatenated; sequence i = ascii[offsets[i] .. offsets[i+1])) into 2 bit-planes per
 * base, chunk-major ([64-base chunk][sequence][lo,hi] -> coalesced 16-B loads across consecutive sequences) and
 * upload them.  Replaces the per-task pickling of Python strings of the reference's Pool fan-out
 * (modules/nearest_neighbor_graph.py:33-35,65; modules/edlib_alignment_module.py:32; modules/SW_alignment_module.py:144).
 * For the nearest-neighbour entry points the sequences MUST be given in the reference's length-sorted order
 * (modules/nearest_neighbor_graph.py:246 / :208).
 */
int isocon_store_create(const uint8_t *ascii, const uint64_t *offsets, uint32_t n, isocon_store **out);
/* The same store from n separate buffers (seq_ptrs[i], seq_lens[i] bytes each): what a host language with its own string objects
 * has -- the library gathers them into its pinned staging buffer while the previous piece is on its way to the device, so the
 * caller does not have to build one contiguous copy first (125 MB at 50 000 x 2.5 kb). */
int isocon_store_create_ptrs(const uint8_t *const *seq_ptrs, const uint64_t *seq_lens, uint32_t n, isocon_store **out);
/* ... with options.  ISOCON_STORE_PRIVATE_SCRATCH: the store keeps a scratch pool of its own (bound matrix, held candidate edges, counters,
 * released with the store) instead of the process-wide one -- for a process that drives SEVERAL searches side by side, each of which
 * expects its scratch to survive the others' calls (the sharded protocol's phases: tests that run the ranks of isocon_amd/dist.py as
 * threads of one process).  One process per GPU -- the reference's Pool workers (modules/nearest_neighbor_graph.py:30-72) are processes
 * too -- needs no flag. */
#define ISOCON_STORE_PRIVATE_SCRATCH 1u
int isocon_store_create_ptrs_ex(const uint8_t *const *seq_ptrs, const uint64_t *seq_lens, uint32_t n, uint32_t flags, isocon_store **out);
/* Pinned host memory for the caller's large input / output buffers (gapped alignments: 2 x 130 MB at 50 000 pairs): copies between
 * the device and these buffers skip the library's staging.  NULL if the allocation fails.  Ordinary memory works everywhere too. */
void *isocon_host_alloc(uint64_t bytes);
void isocon_host_free(void *p);
void isocon_store_destroy(isocon_store *s);
uint32_t isocon_store_size(const isocon_store *s);
/* 64-bit digest of the whole packed set, order-sensitive (computed on the device from the planes and the lengths): the
 * ranks of a sharded run compare it before they split the work (isocon_amd/dist.py). */
int isocon_store_digest(const isocon_store *s, uint64_t *out);
uint64_t isocon_store_device_bytes(const isocon_store *s);
/* Blocking host waits -- synchronous copies and memsets, event and device synchronisations -- of the last nearest-neighbour call on
 * this store (isocon_nn_graph, isocon_nn_partial, isocon_nn_partial_dev): what is left of them is what the search needs an answer
 * from the device for ("How the step is fed to the device"). */
uint64_t isocon_nn_last_host_waits(const isocon_store *s);

/*
 * Batched global (NW) edit distance over an explicit pair list.
 *   k[p] >= 0 : out[p] = distance if <= k[p], else -1      == edlib.align(x, y, mode="NW", task="distance", k=k)
 *               (modules/nearest_neighbor_graph.py:104-107)
 *   k[p] <  0 or k == NULL : unbounded distance            == edlib.align(x, y, "NW")
 *               (modules/edlib_alignment_module.py:111)
 * kernel_ms (optional) receives the summed HIP-event time of the kernels.
 */
int isocon_ed_pairs(isocon_store *s, const uint32_t *a, const uint32_t *b, const int32_t *k, uint64_t n_pairs,
                    int32_t *out_ed, float *kernel_ms);

/*
 * Lower bounds of the pairs' edit distances from q-gram count profiles (isocon_amd/csrc/qgram_mm.hpp: 9-grams hashed into 12288
 * presence bins plus 2 levels of 2048 excess bins; isocon_qgram_params): out_bound[p] <= ed(a[p], b[p]) always.  The main pass of the
 * nearest-neighbour search skips a pair whose bound exceeds its threshold -- the pair edlib would have answered with -1
 * (modules/nearest_neighbor_graph.py:156-162).  The reference has no counterpart; exposed so that the bound can be tested by itself.
 */
/* parameters of the stored q-gram profiles: out[0] = gram length q, out[1] = presence bins, out[2] = excess bins, out[3] = levels kept
 * of an excess bin; returns the binary elements of a profile (out[1] + out[2] * out[3]): the K of the bound kernel's contraction */
int isocon_qgram_params(int32_t *out);
int isocon_qgram_bound_pairs(isocon_store *s, const uint32_t *a, const uint32_t *b, uint64_t n_pairs, int32_t *out_bound);

/*
 * The SECOND lower bound of the main pass, for explicit pairs (tests, diagnostics): out_count[i] = the greedy number of pairwise disjoint
 * 8-grams of sequence partner[i] -- probed at the positions 0, s, 2 s, ... (probe_stride s = 4 or 2: the main pass runs 4 on every pair and 2 on
 * what is left) of the whole 16-base words of the sequence all of whose grams lie inside it -- that
 * occur NOWHERE in sequence owner[i].  Every such gram holds an edited position of any alignment of the two, so out_count[i] <=
 * edit distance; the main pass drops a surviving pair of its q-gram bound whose count exceeds the pair's threshold before any alignment
 * kernel sees it (csrc/nn_filter.hpp).  The reference evaluates those pairs with edlib and gets -1 (modules/nearest_neighbor_graph.py:156-162,
 * :171-178).  Same alphabet rule as isocon_qgram_bound_pairs.
 */
int isocon_block_bound_pairs(isocon_store *s, const uint32_t *owner, const uint32_t *partner, uint64_t n_pairs, int32_t probe_stride, int32_t *out_count);

/*
 * The two kernels of the main pass that APPLY that bound (csrc/nn_filter.hpp: k_nn_block_filter, k_nn_block_filter2), run on chunks the
 * caller made (tests): the launches, grids and buffer layout are the main pass's own.  The reference has no counterpart.
 *   thr[i], i < store size     threshold of entry i, 0 .. 64 (the 7-bit field of the main pass's per-entry word)
 *   chunk c < n_chunks         owner[c], narrow[c] (0: 64-row class, 1: 32-row class), list words words[chunk_ptr[c] .. chunk_ptr[c + 1]):
 *                              1 .. 2111 of them (what the list builder hands over: its chunk size + 63); chunk_ptr[0] = 0.  A list word is
 *                              partner | bit 30 (the owner's threshold applies) | bit 31 (the partner's applies); the pair's threshold is
 *                              min(kcap, the larger of those that apply), -1 with neither bit.
 *   kcap, list_min (>= 1), second_pass (0 / 1)
 * A pair survives the first pass iff count(owner, partner, stride 4) <= its threshold.  With np survivors of a chunk of `count` pairs:
 * np >= list_min and (no second pass or 2 np >= count): they stay a chunk of the chunk's class; else, with the second pass and np >= 16,
 * they pass it (64 per task; survivors: count(.., stride 2) <= threshold as well) to the flat pairs; else they join the flat pairs as they are.
 * Out: the chunks left, the 64-row class first -- out_slot / out_count / out_begin[i], i < out_counters[0] + out_counters[1], their words at
 * out_list[out_begin[i] ..) in no defined order (out_list: all chunk_ptr[n_chunks] words of the list after the passes); the flat pairs
 * out_pa / out_pb[i], i < out_counters[2], in no defined order.  out_counters[9] = chunks left of the 64-row class, of the 32-row class, flat
 * pairs, pairs rejected by the first pass, by the second, pairs in the chunks left, of those in 32-row chunks, tasks of the second pass, the
 * kernels' overflow word (always 0: the device buffers hold the worst case).
 * ISOCON_E_ARG: an index out of range, a chunk of 0 or more than 2111 words, thr outside 0 .. 64, chunks_cap < n_chunks, list_cap or
 * pairs_cap < chunk_ptr[n_chunks] (every pair kept), sequences of 16384 bases or more.  Same alphabet rule as isocon_qgram_bound_pairs.
 */
int isocon_block_filter_chunks(isocon_store *s, const int32_t *thr, uint32_t n_chunks, const uint32_t *owner, const uint8_t *narrow, const uint64_t *chunk_ptr,
                               const uint32_t *words, int32_t kcap, uint32_t list_min, int32_t second_pass, uint32_t *out_slot, uint32_t *out_count,
                               uint64_t *out_begin, uint64_t chunks_cap, uint32_t *out_list, uint64_t list_cap, uint32_t *out_pa, uint32_t *out_pb, uint64_t pairs_cap,
                               uint64_t *out_counters);

/*
 * The block test of the depth-limited 2-set search (csrc/nn2_depth.hpp: k_nn2_block_reject) on pairs the caller made (tests): the kernel
 * and its launch are the search's own.  Pair p = (read[p], target[p]) with threshold k[p]; runs of equal read[] are one read's pairs of a
 * round and are cut into tasks of at most 64 pairs, a wave each (the search itself lists at most 33 per read and round).
 * out_rejected[p] = 1 iff the pair is tested and isocon_block_bound_pairs(read[p], target[p], probe_stride) > k[p] -- its distance then
 * exceeds k[p] --, else 0.  Not tested: k[p] < 0 (how the search marks a pair outside the planes' map), a pair with a sequence that holds
 * symbols outside the 2-bit map (whatever k[p]; no ISOCON_E_ALPHABET), and k[p] >= len(target[p]) / 8 (the count cannot exceed it).
 * *kernel_ms (may be NULL): HIP-event time of the test's launch.  ISOCON_E_ARG: an index >= the store's size, probe_stride other than 2
 * or 4, 2^31 pairs or more.  The reference has no counterpart: it aligns these pairs and gets -1 (modules/nearest_neighbor_graph.py:341-424).
 */
int isocon_nn2_block_reject(isocon_store *s, const uint32_t *read, const uint32_t *target, const int32_t *k, uint64_t n_pairs, int32_t probe_stride,
                            uint8_t *out_rejected, float *kernel_ms);

/*
 * The bound matrix the main pass of isocon_nn_graph / isocon_nn_partial consults for the shard (q_begin, q_end, q_stride, q_block) --
 * see isocon_nn_partial -- of a length-sorted store, read back for tests: row r belongs to the shard's r-th entry q, its bytes
 * out_bounds[out_row_ptr[r] .. out_row_ptr[r + 1]) are min(255, bound) of the pairs (q, p), p = q + 1, q + 2, ... while
 * len(p) - len(q) <= 63 and p - q <= depth (the pairs the upward scan of modules/nearest_neighbor_graph.py:136-153 can reach within
 * 63 edits).  out_row_ptr has (number of rows + 1) entries.  ISOCON_E_CAPACITY + *n_bounds_needed when bounds_cap is too small.
 */
int isocon_qgram_bound_matrix(isocon_store *s, uint32_t q_begin, uint32_t q_end, uint32_t q_stride, uint32_t q_block, uint64_t depth,
                              uint64_t *out_row_ptr, uint8_t *out_bounds, uint64_t bounds_cap, uint64_t *n_bounds_needed);

/*
 * What the bound kernel leaves BESIDE that matrix for a search over the shard with the roles is_converged / is_target (each may be NULL,
 * as for isocon_nn_graph) and the seed pairs proposed from it, read back raw for tests: the launches are the search's own up to the
 * proposal of the seed pairs; no pair is aligned.  The reference has no counterpart.  With rows = the entries of the shard and
 * S = out_params[0]:
 *   out_score[n]               hub scores: window pairs with a bound <= out_params[1] that have the entry at either end
 *   out_rowmin[rows * S]       per row and class c of column tiles ((p / out_params[2]) % S == c): the smallest (bound, column) over the
 *                              row's admissible columns as bound << 32 | (p - q - 1); all ones: none
 *   out_colmin[n * S]          per entry p and class c of ROW tiles ((slot / out_params[2]) % S == c): the smallest (bound, row entry) over
 *                              the admissible rows whose window holds p as bound << 32 | q; all ones: none
 *   out_pa, out_pb[2 * S * n]  the proposed pairs, *out_count of them in no defined order, 0xffffffff behind them
 *   out_known[n * 2 * S]       per entry the other ends of the pairs it proposed, in the order it proposed them, then 0xffffffff
 *   out_params[4]              S (seed classes), the hub bound, the tile size, and the number of merged column classes of the proposal
 * With every output but out_params NULL the call only fills out_params[0 .. 2] (the sizes above).  ISOCON_E_UNSUPPORTED: no room for
 * the matrix, the minima or the table of the seed pairs.  Argument and alphabet errors as isocon_qgram_bound_matrix.
 */
int isocon_qgram_seed_tables(isocon_store *s, const uint8_t *is_converged, const uint8_t *is_target, uint64_t depth,
                             uint32_t q_begin, uint32_t q_end, uint32_t q_stride, uint32_t q_block,
                             uint32_t *out_score, uint64_t *out_rowmin, uint64_t *out_colmin, uint32_t *out_pa, uint32_t *out_pb,
                             uint64_t *out_count, uint32_t *out_known, uint32_t *out_params);

/* statistics block filled by the nearest-neighbour entry points (all counters are for the one call) */
typedef struct {
    uint64_t pairs_evaluated;     /* (shared,lane) pairs the banded kernels actually ran */
    uint64_t cells_columns;       /* text columns processed, summed over evaluated lanes (lanes x wave columns) */
    uint64_t live_columns;        /* ... counting a lane only while its pair was still undecided */
    uint64_t tiles;               /* 64-lane tiles executed */
    uint64_t hits;                /* candidate edges recorded on the device */
    uint64_t fallback_queries;    /* queries that needed a band wider than 64 rows */
    uint64_t full_pairs;          /* pairs sent to the un-banded kernel (filled by the depth-limited 2-set search as well) */
    float kernel_ms;              /* HIP-event time of all kernels of the call */
    float scan_kernel_ms;         /* ... of the dominant kernel launch (64-row band scan, main pass) */
    float seed_kernel_ms;         /* ... of the seed pass that precedes it (1-set only) */
    uint32_t scan_launches;       /* launches summed into scan_kernel_ms; depth-limited 2-set search: the number of rounds (see isocon_nn_graph) */
    uint64_t pairs_prefiltered;   /* pairs of the main pass whose q-gram bound exceeded their threshold (never aligned) */
    float bound_kernel_ms;        /* HIP-event time of the q-gram profile + bound kernels (part of kernel_ms) */
    float list_kernel_ms;         /* ... of the kernel that collects the survivors of the bounds into lists (part of kernel_ms) */
    float lanes_kernel_ms;        /* ... of the one-pair-per-lane launch of the main pass (entries with few pairs; NOT in scan_kernel_ms) */
    float narrow_kernel_ms;       /* of scan_kernel_ms: the table launch over the pairs whose threshold is <= 31 (32-row form of the kernel) */
    uint64_t pairs_lanes;         /* pairs of the main pass aligned one pair per lane (the rest went through tables); depth-limited 2-set search: see isocon_nn_graph */
    uint64_t bound_tiles;         /* 256 x 256 tiles of the bound matrix computed (each: 65 536 pairs x isocon_qgram_params() multiply-adds) */
    uint64_t pairs_wide_to_lanes; /* of pairs_lanes: pairs with a threshold above 31 sent there because of it (ISOCON_DEBUG_VARIANT=nn_narrow=1 only) */
    uint64_t narrow_columns;      /* of cells_columns: columns run by the 32-row form of the table kernel */
    uint64_t pairs_narrow;        /* pairs listed in chunks of the 32-row class */
    uint64_t pairs_bytes;         /* pairs with a sequence that holds symbols outside the 2-bit map, aligned on the bytes (see "Alphabet") */
    uint64_t pairs_block_rejected;/* survivors of the q-gram bound that the block filter rejected (greedy count of disjoint absent 8-grams > threshold; never aligned) */
    float filter_kernel_ms;       /* HIP-event time of the block filter (part of list_kernel_ms) */
    float mm_kernel_ms;           /* ... of the bound matrix contraction k_qgram_mm alone (part of bound_kernel_ms) */
    uint64_t pairs_seed_known;    /* of pairs_lanes: pairs the seed pass of the same call had aligned already (their outcome is final: not aligned again, unless ISOCON_DEBUG_VARIANT=nn_seed_skip=0 / =count) */
    uint64_t pairs_lanes_aligned; /* pairs the one-pair-per-lane launch of the main pass ran: pairs_lanes - pairs_seed_known (pairs_lanes with nn_seed_skip=0 / =count) */
} isocon_nn_stats;

/*
 * Exact nearest-neighbour graph over a length-sorted store.
 *   1-set (is_target == NULL): for every i with is_converged[i] == 0 the arg-min set of POSITIVE edit distances
 *     over all other sequences, restricted to d <= len(i) and to sorted-order offsets <= depth
 *     == get_nearest_neighbors (modules/nearest_neighbor_graph.py:110-198) for every query, i.e. the whole of
 *     get_exact_nearest_neighbor_graph (:19-82) independent of nr_cores.
 *   2-set (is_target != NULL): queries are the entries with is_target[i] == 0, neighbours only entries with
 *     is_target[i] == 1, distance 0 admitted == get_nearest_neighbors_2set (:341-424).
 *     depth >= the number of targets (the reference's default 2**32) never binds.  A smaller depth is the reference's rule (:416): a
 *     read stops after the iteration in which its count of candidate alignments reaches depth (depth + 1 alignments at most, depth 0 =
 *     one iteration), candidates visited by ascending offset, the lower one first -- carried out on the device round by round.
 *     Under ISOCON_DEBUG_VARIANT=nn2_block_filter (off by default: it costs more than it saves, profiles/nn2set_depth.txt; off under
 *     nn_no_block_filter in any case) a listed pair whose block bound (isocon_block_bound_pairs, stride 2) exceeds its threshold is
 *     final with the -1 edlib would give and is not aligned (csrc/nn2_depth.hpp, k_nn2_block_reject): same rows.
 *     stats on that path: kernel_ms, hits, pairs_lanes = distinct (read, candidate) pairs whose distance was asked for (the same with
 *     and without the block test), pairs_block_rejected = of those, pairs the block test decided, pairs_lanes_aligned = pairs handed to
 *     the one-pair-per-lane launch (pairs_lanes - pairs_block_rejected), filter_kernel_ms = HIP-event time of the test's launches
 *     (2-bit texts, test, compaction, scatter; part of kernel_ms), full_pairs, pairs_bytes (never tested, never rejected),
 *     scan_launches = rounds.
 * Output CSR: out_best[i] = minimal distance (-1 if row empty), out_row_ptr[n+1], out_cols = neighbour indices in
 * the reference's insertion order (ascending offset, lower index first).  If the edges do not fit cols_cap the
 * call returns ISOCON_E_CAPACITY and *n_cols_needed holds the required capacity.
 */
int isocon_nn_graph(isocon_store *s, const uint8_t *is_converged, const uint8_t *is_target, uint64_t depth,
                    int32_t *out_best, uint64_t *out_row_ptr, uint32_t *out_cols, uint64_t cols_cap,
                    uint64_t *n_cols_needed, isocon_nn_stats *stats);

/*
 * Sharded variant for one-process-per-GPU runs (the reference has no distributed path; its Pool chunking is
 * modules/nearest_neighbor_graph.py:33-35).  A rank OWNS the entries x of the length-sorted order with q_begin <= x < q_end and
 * (x - q_begin) mod q_stride < q_block (q_block a power of two, 1 <= q_block <= q_stride):
 *     rank r of N, block-cyclic:  q_begin = 256 r, q_end = n, q_stride = 256 N, q_block = 256 -- blocks of 256 consecutive entries
 *                                 (one tile row of the bound matrix) dealt round-robin: the very uneven windows balance by themselves
 *                                 and a rank's tiles stay as dense as on one GPU (what isocon_amd/dist.py uses);
 *     cyclic:                     q_begin = r, q_stride = N, q_block = 1;       contiguous: q_stride = q_block = 1.
 * best_inout[n] is IN/OUT (0x3fffffff = no neighbour known yet).
 *   phase 0: seed pass -- every owned entry against its 64 nearest longer neighbours (64-row band).  Pass best_inout all
 *            0x3fffffff.  (No-op for the 2-set graph.)
 *   phase 1: 64-row band over every remaining admissible pair whose LOWER index is owned (1-set and 2-set alike;
 *            only the long-read fallback of the 2-set search assigns a pair to the rank that owns its read);
 *            best_inout = element-wise MIN over all ranks' phase-0 results (tight thresholds on every rank).
 *   phase 3: phases 0 and 1 in one call, no exchange between them (single-rank callers; with several ranks the seeds of a rank's
 *            own rows leave its thresholds loose: summed work x 2 to x 4 on C3, which is why isocon_amd/dist.py reduces after phase 0).
 *   phase 2: 128/256/512-row bands over the pairs whose lower index is owned and that involve an entry still
 *            unresolved in best_inout (= MIN over all ranks' phase-1 results), then the un-banded kernel for the owned
 *            queries whose neighbour is further than 511 edits.  wide_queries (phase 2 only; NULL = the entries that are unresolved
 *            at the call): the queries of the WHOLE phase when the caller runs it in sub-steps over sub-shards with a reduction of
 *            best_inout after each (isocon_amd/dist.py does: a query's threshold then has seen part of its pairs on ALL ranks from
 *            the second sub-step on) -- wide_queries[i] != 0 for the entries that were unresolved when the phase began.
 * Each call returns up to hits_cap candidate edges (endpoint, neighbour, distance) as int32 triples.  The caller
 * min-reduces best over ranks after each phase, all-gathers the triples and calls isocon_nn_finalize.
 */
int isocon_nn_partial(isocon_store *s, const uint8_t *is_converged, const uint8_t *is_target, uint64_t depth,
                      uint32_t q_begin, uint32_t q_end, uint32_t q_stride, uint32_t q_block, int32_t phase, int32_t *best_inout,
                      int32_t *out_hits, uint64_t hits_cap, uint64_t *n_hits, isocon_nn_stats *stats, const uint8_t *wide_queries);
int isocon_nn_finalize(uint32_t n, const int32_t *best, const int32_t *hits, uint64_t n_hits,
                       int32_t *out_best, uint64_t *out_row_ptr, uint32_t *out_cols, uint64_t cols_cap,
                       uint64_t *n_cols_needed);

/*
 * The same protocol with the exchanged data resident in device memory (what isocon_amd/dist.py uses on a GPU: RCCL reduces and
 * gathers device buffers, nothing crosses PCIe between the exchange steps but a few status words).  All work is issued on the
 * NULL stream of the current device; pointers named *_dev are device pointers owned by the caller.
 *   isocon_nn_partial_dev  one phase like isocon_nn_partial; best_inout_dev[n] is read and updated in place; the phase's candidate
 *                          edges are appended to a list the library keeps in device memory (keep_hits 0: the list starts empty --
 *                          pass 0 for the first phase of a search); *n_hits_held = edges held after the call.
 *   isocon_nn_hits_dev     writes the held edges that attain best_dev[] of their endpoint to out_hits_dev (int32 triples), the
 *                          rest of the cap_rows rows as (-1, -1, -1): a fixed-size block for one all_gather.  cap_rows must be >=
 *                          the number of edges held (ISOCON_E_CAPACITY otherwise).
 *   isocon_nn_finalize_dev isocon_nn_finalize from device buffers (rows with a negative endpoint are skipped); n = size of the store.
 */
int isocon_nn_partial_dev(isocon_store *s, const uint8_t *is_converged, const uint8_t *is_target, uint64_t depth,
                          uint32_t q_begin, uint32_t q_end, uint32_t q_stride, uint32_t q_block, int32_t phase, int32_t *best_inout_dev,
                          int32_t keep_hits, uint64_t *n_hits_held, isocon_nn_stats *stats, const uint8_t *wide_queries);
int isocon_nn_hits_dev(isocon_store *s, const int32_t *best_dev, int32_t *out_hits_dev, uint64_t cap_rows, uint64_t *n_kept);
int isocon_nn_finalize_dev(isocon_store *s, const int32_t *best_dev, const int32_t *hits_dev, uint64_t n_rows,
                           int32_t *out_best, uint64_t *out_row_ptr, uint32_t *out_cols, uint64_t cols_cap, uint64_t *n_cols_needed);

/*
 * Batched semi-global affine alignment with traceback == parasail.sg_trace_scan_16/32(s1=a, s2=b, open, ext,
 * matrix_create("ACGT", match, mismatch)) + the CIGAR decode and column counting of parasail_alignment
 * (modules/SW_alignment_module.py:64-86).  mismatch is per pair (the reference picks it from the error-rate
 * bucket, :102-109).  tie_policy 0 = parasail's behaviour as restated in oracle/isocon_oracle.c.
 * Outputs: CIGAR ops as (len << 4 | code), code 0 '=', 1 'X', 2 'I' (consumes a), 3 'D' (consumes b);
 * out_ops_ptr[n_pairs+1]; out_res[6*p..] = score, end_query, end_ref, matches, mismatches, indels.
 * ed_upper (may be NULL; entries < 0 = unknown): an upper bound of the pair's edit distance -- the reference's
 * sw_align_sequences receives exactly that in its input dict (modules/SW_alignment_module.py:89-101).  It only
 * narrows the part of the DP matrix that is computed; the result is always the full-matrix result: a banded alignment
 * is accepted only if its score proves that nothing outside the band can reach it, otherwise the pair is redone in full.
 */
int isocon_sg_trace_batch(isocon_store *s, const uint32_t *a, const uint32_t *b, uint64_t n_pairs, int32_t match,
                          const int8_t *mismatch_per_pair, int32_t open, int32_t ext, int32_t tie_policy,
                          uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap, uint64_t *n_ops_needed,
                          int32_t *out_res, float *kernel_ms, const int32_t *ed_upper);

/*
 * Same as isocon_sg_trace_batch plus the two gapped strings per pair (what cigar_to_seq builds from the CIGAR in the
 * reference, modules/SW_alignment_module.py:15-56,78): out_aln_a / out_aln_b hold, for pair p, the bytes
 * [out_aln_ptr[p], out_aln_ptr[p+1]) = the aligned query / reference with '-' for gaps (equal lengths).
 * ISOCON_E_CAPACITY + *n_aln_needed when aln_cap is too small.  Both sequences of every pair must be non-empty.
 */
int isocon_sg_strings_batch(isocon_store *s, const uint32_t *a, const uint32_t *b, uint64_t n_pairs, int32_t match,
                            const int8_t *mismatch_per_pair, int32_t open, int32_t ext, int32_t tie_policy,
                            uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap, uint64_t *n_ops_needed,
                            int32_t *out_res, uint8_t *out_aln_a, uint8_t *out_aln_b, uint64_t *out_aln_ptr,
                            uint64_t aln_cap, uint64_t *n_aln_needed, float *kernel_ms, const int32_t *ed_upper);

/*
 * Where the kernel time of this thread's most recent isocon_sg_trace_batch / isocon_sg_strings_batch call went (HIP events on the
 * kernels' stream; a measurement aid for bench.py's `roofline_sw`, the reference has no counterpart: parasail's time is one number per
 * call, modules/SW_alignment_module.py:66-69).  out[0 .. min(cap, 11)): forward kernels (k_sg_band + k_sg_forward) ms, walk kernels ms,
 * compaction ms, string expansion ms, pairs aligned with the band's diagonals on the lanes, pairs aligned in strips, pairs whose
 * banded result could not be certified and was redone in full, bytes of trace scratch the forward kernels wrote, pairs of the fifth
 * value that ran on 128 diagonals (two per lane instead of four), those of them whose bound asks for more than 128 diagonals (run
 * narrower first: the certificate decides), and those of these that failed it and ran again in the band of their bound.  Returns the
 * number of values written.
 */
int isocon_sg_last_stats(double *out, int32_t cap);

/*
 * Exon-difference filter on CIGAR ops (host-only helper, no GPU): out_flag[p] = 1 iff filter_exon_differences
 * (modules/functions.py:23-50, mask rule :218-236) would drop the pair, i.e. one of the gapped strings has a run of
 * >= min_exon_diff gaps inside the window that excludes min(ignore_ends_len, end-gap) columns at either end.
 * ops / ops_ptr as returned by isocon_sg_trace_batch.
 */
int isocon_exon_filter_from_ops(const uint32_t *ops, const uint64_t *ops_ptr, uint64_t n_pairs, int32_t min_exon_diff,
                                int32_t ignore_ends_len, uint8_t *out_flag);

/* Consensus correction of one partition on its multi-alignment matrix -- replaces the column statistics and the
 * per-read correction of modules/correction_module.py:277-402 (position frequency matrix modules/functions.py:526-536).
 * matrix: n_rows x n_cols bytes, row-major, symbols 'A' 'C' 'G' 'T' '-' (layout of functions.create_multialignment_matrix);
 * degree[r]: multiplicity of row r (rows with degree > 1 are counted degree times and never corrected).
 * Per column: weighted counts, majority symbol (first maximum in the order A, C, G, T, -), unambiguous iff unique.
 * Per row of degree 1: the positions where an unambiguous majority differs from the row are correctable; with
 * frequency = count of the row's symbol in the column / partition total of that error class (insertion, deletion,
 * substitution; over the unambiguous columns; at least 1), every position whose frequency is <= the ceil(n/2)-th
 * smallest is replaced by the majority.  Output: the corrected rows without their '-' symbols, packed
 * (out_offsets[n_rows + 1]), out_n_cand[r] = number of correctable positions (rows with more than the 2048 the kernel
 * keeps in LDS are run again with their list in HBM), out_class_totals[3] = insertion, deletion, substitution totals.
 * The matrix is handled as a batch of one partition by the kernels of the batched entry points below (csrc/msa.hpp).
 * ISOCON_E_CAPACITY if packed_cap is too small (out_offsets[n_rows] holds the size needed). */
int isocon_msa_correct(const uint8_t *matrix, uint32_t n_rows, uint32_t n_cols, const int32_t *degree,
                       uint8_t *out_packed, uint64_t packed_cap, uint64_t *out_offsets, int32_t *out_n_cand,
                       int64_t *out_class_totals, float *kernel_ms);

/*
 * The same correction with the multi-alignment matrix built ON THE DEVICE from the alignments' CIGAR ops (f1 + f3 fused with a12-a15:
 * the gapped strings of sw_align_sequences never exist).  Replaces modules/functions.py:543-588 (create_multialignment_matrix),
 * :598-631 (position_query_to_alignment) and the column layout of :679-767 for the partitions of get_partition_alignments
 * (modules/isocon_get_candidates.py:37-81) + correct_strings (modules/correction_module.py:12-75).
 *   isocon_msa_build_ops      rows = the partition: row_ids[0] the centre, row_ids[1 ..] its members (ids of the store); the ops of row r
 *                             (isocon_sg_trace_batch's encoding; centre = QUERY of the alignment) are ops[ops_ptr[r] .. ops_ptr[r + 1]),
 *                             ops_ptr[0] = ops_ptr[1] = 0.  Builds the matrix in device memory (kept for the call below) and returns
 *                             *out_n_cols, out_col_slot[len(centre) + 1] (first column of every insertion slot; optional),
 *                             out_longest[len(centre) + 1] (longest insertion per slot; optional) and the insertions of the WIDE slots
 *                             (longest >= 2) as records of 8 uint32 (row, slot, first position in the member, length, the 2-bit codes
 *                             A C G T = 0 1 2 3 of its first 32 bases in two words, two spare words): where those sit inside
 *                             their slot is decided by the reference's string heuristics (get_best_solution, functions.py:635-676),
 *                             which the Python layer applies and hands back as patches.  ISOCON_E_CAPACITY + *n_wide if wide_cap is
 *                             too small; ISOCON_E_ARG if the ops of a row do not spell both sequences.
 *   isocon_msa_correct_built  patches (patch_bytes[patch_ptr[i] .. patch_ptr[i + 1]) into row patch_row[i] from column patch_col[i]),
 *                             then isocon_msa_correct on the built matrix (same outputs).  One build serves one correction.
 *   isocon_msa_read_built     the built matrix (tests).
 * These are the batched entry points below on a batch of one partition (same kernels; word 6 of a wide record, the partition, is 0).  A
 * build pairs only with the correction of its own kind: isocon_msa_correct_built / isocon_msa_read_built after isocon_msa_build_ops_batch
 * is ISOCON_E_ARG, and so is isocon_msa_correct_built_batch after isocon_msa_build_ops.  isocon_msa_correct on the process' scratch pool
 * uses the slots of a build in that pool: such a build is no longer there afterwards.
 */
int isocon_msa_build_ops(isocon_store *s, uint32_t n_rows, const uint32_t *row_ids, const uint32_t *ops, const uint64_t *ops_ptr,
                         uint32_t *out_n_cols, uint32_t *out_col_slot, uint32_t *out_longest, uint32_t *out_wide, uint64_t wide_cap,
                         uint64_t *n_wide, float *kernel_ms);
int isocon_msa_correct_built(isocon_store *s, uint32_t n_rows, uint32_t n_cols, const uint32_t *patch_row, const uint32_t *patch_col,
                             const uint32_t *patch_ptr, const uint8_t *patch_bytes, uint32_t n_patches, const int32_t *degree,
                             uint8_t *out_packed, uint64_t packed_cap, uint64_t *out_offsets, int32_t *out_n_cand,
                             int64_t *out_class_totals, float *kernel_ms);
int isocon_msa_read_built(isocon_store *s, uint32_t n_rows, uint32_t n_cols, uint8_t *out_matrix);

/*
 * The same two steps for ALL partitions of a correction step at once (correct_strings, modules/correction_module.py:12-75, loops over the
 * partitions -- a Pool task each; later steps of a run have hundreds to thousands of small partitions).  Rows of all partitions are
 * concatenated: partition p = rows first_row[p] .. first_row[p + 1] (its first row is the centre, with no ops), row_ids / ops_ptr / degree
 * index the concatenation, the slot arrays (out_col_slot, out_longest) are concatenated too (len(centre) + 1 entries per partition, in
 * partition order).  Wide records as in isocon_msa_build_ops with the row as an index into the concatenation and the partition in word 6;
 * patches address (row of the concatenation, column of that row's matrix).  out_n_cand[r] = -1 for a row with more correctable positions
 * than the 1024 the kernel keeps in LDS in this call: its partition has to be corrected through the single-partition entry points (its output
 * rows are not valid).  If packed_cap is too small (ISOCON_E_CAPACITY, out_offsets[n_rows] holds the size needed) the build stays: call again.
 */
int isocon_msa_build_ops_batch(isocon_store *s, uint32_t n_parts, const uint32_t *first_row, const uint32_t *row_ids, const uint32_t *ops,
                               const uint64_t *ops_ptr, uint32_t *out_n_cols, uint32_t *out_col_slot, uint32_t *out_longest, uint32_t *out_wide,
                               uint64_t wide_cap, uint64_t *n_wide, float *kernel_ms);
int isocon_msa_correct_built_batch(isocon_store *s, uint32_t n_parts, uint32_t n_rows, const uint32_t *patch_row, const uint32_t *patch_col,
                                   const uint32_t *patch_ptr, const uint8_t *patch_bytes, uint32_t n_patches, const int32_t *degree,
                                   uint8_t *out_packed, uint64_t packed_cap, uint64_t *out_offsets, int32_t *out_n_cand, float *kernel_ms);

/*
 * The two builds with the insertions of the wide slots PLACED ON THE DEVICE: get_best_solution (functions.py:635-676 with min_ed
 * :771-799) for every slot whose longest insertion has at most 62 bases ('-' + longest + '-' then fits the 64 lanes of a wavefront;
 * csrc/msa_place_core.hpp states the rule, k_msa_slot_rep / k_msa_place of csrc/msa.hpp apply it).  Arguments and refusals as
 * isocon_msa_build_ops / isocon_msa_build_ops_batch without the record list: the list stays on the device (sized from the code-3 ops, so
 * no capacity of it is the caller's business) and the placements are in the built matrix when the call returns.  What comes back are the
 * records of the slots with a longest insertion beyond 62 bases only -- ALL records of such a slot, for the representative is picked from
 * them -- in out_left (8 words each, the format of the builds above; *n_left of them, in no particular order; normally none), to be
 * placed by the caller and sent as patches to isocon_msa_correct_built / isocon_msa_correct_built_batch, which pair with these builds
 * as with the builds above (isocon_msa_read_built too).  *n_placed = records placed on the device (duplicates counted): *n_placed +
 * *n_left is the *n_wide of the builds above.  ISOCON_E_CAPACITY if left_cap is too small: *n_left holds the count and the build STAYS
 * (the matrix is complete but for the left-over records); the caller calls again for the list, which builds the same matrix again.
 */
int isocon_msa_build_ops_placed(isocon_store *s, uint32_t n_rows, const uint32_t *row_ids, const uint32_t *ops, const uint64_t *ops_ptr,
                                uint32_t *out_n_cols, uint32_t *out_col_slot, uint32_t *out_longest, uint32_t *out_left, uint64_t left_cap,
                                uint64_t *n_left, uint64_t *n_placed, float *kernel_ms);
int isocon_msa_build_ops_placed_batch(isocon_store *s, uint32_t n_parts, const uint32_t *first_row, const uint32_t *row_ids, const uint32_t *ops,
                                      const uint64_t *ops_ptr, uint32_t *out_n_cols, uint32_t *out_col_slot, uint32_t *out_longest, uint32_t *out_left,
                                      uint64_t left_cap, uint64_t *n_left, uint64_t *n_placed, float *kernel_ms);

/*
 * Batched infix ("HW") edit distance with location and path ends == edlib.align(q, t, mode="HW", task="path", k=k)
 * as consumed by edlib_traceback (modules/end_invariant_functions.py:593-620) inside get_all_NN (:622-681), the
 * candidate-vs-candidate graph of the statistical-test phase: the query is aligned globally inside the target, target
 * prefix and suffix are free.  k[p] >= 0 is required (k = 10 + ignore_ends_len there); the diagonals a path of cost <= k
 * can visit must fit 512 (max(len(t) - len(q), 0) + 2 k + 1 <= 512), otherwise ISOCON_E_UNSUPPORTED.
 * out[5 p ..] = editDistance (-1 if > k[p]; then the rest is -1 / 0), locations[0] start, end (0-based, inclusive: the
 * first optimal end, the smallest start for it), length of the insertion run (query bases without target) the path
 * starts with, length of the one it ends with (0 = the CIGAR does not start / end with 'I').  Path = global alignment of
 * q to t[start..end], traced from the end preferring I, then D, then the diagonal (oracle/isocon_oracle.c section 5).
 */
int isocon_hw_pairs(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                    int32_t *out, float *kernel_ms);

/*
 * Which route and band classes the calling thread's last isocon_hw_pairs call took (no counterpart in the reference; tests).
 * out[0] route (0: tiles built on the host, 1: on the device); out[1] 1 if the call fell back from device tiles to host tiles;
 * out[2] pairs of the call; out[3] pairs that needed a kernel; out[4] hits; out[5..8] LOCATE tiles of the classes of 1, 2, 4 and 8
 * window words (64, 128, 256, 512 diagonals; on the device route a tile is filed under the class of its COMMON window);
 * out[9..12] START + TRACE tiles per class; out[13..16] the grid each of those launches got (fewer workgroups than tiles: a
 * workgroup ran several tiles on one store).  isocon_hw_pairs zeroes the values when it is called.  isocon_hw_window_graph and
 * isocon_hw_path_pairs run the device route on lists of their own and leave its counters here, with out[3] = out[4] = -1 (not
 * counted).  Writes min(cap, 17) values and returns that number.
 */
int isocon_hw_last_stats(double *out, int32_t cap);

/*
 * isocon_hw_pairs without the limit of 512 diagonals: the same arguments, checks and (n_pairs, 5) output, for any k[p] <= 2^20 --
 * edlib_traceback (modules/end_invariant_functions.py:593-620) with k >= 256, and get_all_NN (:661, :668: k = 10 + ignore_ends_len over
 * a length window of 10 + 2 ignore_ends_len) with ignore_ends_len >= 121.  Every pair is classed on the host from the two lengths and
 * k[p]: the pairs isocon_hw_pairs accepts go through it as one sub-list (their rows are the rows it returns; a call without any other
 * pair IS that call), the others through un-banded kernels (one wavefront per pair, the whole query in 64-row blocks).  The vectors
 * the path walk needs are kept per launch in at most 1 GiB of scratch: the wide pairs are cut into as many launches as that takes, and
 * a single pair that needs more on its own is refused with ISOCON_E_UNSUPPORTED (isocon_last_error states its sizes).  So is a query of
 * more than 4 096 bases against a target of more than 655 360.  *kernel_ms sums both parts.
 */
int isocon_hw_pairs_wide(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                         int32_t *out, float *kernel_ms);

/*
 * The candidate-vs-candidate graph with ignored ends from the store alone: the pair list of get_all_NN
 * (modules/end_invariant_functions.py:622-681), the end rules of edlib_traceback (:593-620) and, with symmetric != 0, the symmetrisation
 * of get_NN_graph_ignored_ends_edlib (:757-788) on the device -- no pair list goes up, no per-pair rows come down.
 * The store must be in ascending length order (ISOCON_E_ARG otherwise).  Entry i visits the offsets j = 1, 2, ... (i - j before i + j;
 * a side ends for good at the first length difference above `window` or at the list's end; the offsets stop at max(1, min(depth, n))).
 * Every visited pair (query i inside target t) gets the row isocon_hw_pairs returns for it with threshold k, and from it
 *   adj = ed + max(0, start - T) + max(0, len_t - (end + 1) - T) - min(trailing I run, T) - min(leading I run, T),  T = end_threshold;
 * i -> t is a directed edge iff ed >= 0 and 0 <= adj <= max_ed.  Row i = out_cols / out_ed [out_row_ptr[i] .. out_row_ptr[i + 1]):
 *   symmetric == 0: the directed edges of i in visit order with adj (get_all_NN on the whole list);
 *   symmetric != 0: the directed edges of i in visit order, each with min(adj(i -> t), adj(t -> i)) where t -> i is a directed edge too,
 *     then every t with a directed edge t -> i and none i -> t, in ascending t with adj(t -> i) (the dict of dicts the reference ends
 *     with, insertion order included).
 * Limits: window + 2 k + 1 <= 512 diagonals and at most 0xfffffff0 pairs, else ISOCON_E_UNSUPPORTED (so when the tiles cannot be formed
 * on the device); a store of more than four symbols ISOCON_E_ALPHABET, with the message of isocon_hw_pairs; negative parameters
 * ISOCON_E_ARG.  ISOCON_E_CAPACITY + *n_edges_needed when edges_cap is too small (out_row_ptr and the counters are valid then); the
 * number of ordered window pairs bounds the edges in both forms.
 * out_counters (5 values, or NULL): pairs, pairs that needed a kernel, hits (ed >= 0), directed edges, appended entries (second part of
 * the symmetric rows).  *kernel_ms sums the enumeration, alignment and edge kernels.
 */
int isocon_hw_window_graph(isocon_store *s, int32_t window, int32_t k, uint64_t depth, int32_t end_threshold, int32_t max_ed,
                           int32_t symmetric, uint64_t *out_row_ptr /* n + 1 */, uint32_t *out_cols, int32_t *out_ed,
                           uint64_t edges_cap, uint64_t *n_edges_needed, uint64_t *out_counters, float *kernel_ms);

/*
 * The invariance graph of the end-invariant collapse from the store alone: the pairs and the test of
 * get_invariants_under_ignored_edge_ends_speed (modules/end_invariant_functions.py:920-951, is_overlap :884-918) on the device -- no
 * sequence is compared on the host.  The store must be in ascending length order (ISOCON_E_ARG otherwise; so is thr < 0).
 * Row i = out_cols[out_row_ptr[i] .. out_row_ptr[i + 1]): the positions p != i with len_i - 2 thr <= len_p <= len_i (equal lengths are
 * visited from both sides) for which the reference's test of (seq1 = i, seq2 = p) holds, in ascending p:
 *   p occurs inside i: its FIRST occurrence decides -- at most thr symbols of i before and after it -- and nothing else is tried;
 *   otherwise a suffix of one equals a prefix of the other and leaves at most thr symbols of either uncovered.
 * Both are "the two coincide on their whole overlap under one of at most 2 thr + 1 shifts" (csrc/end_inv_core.hpp): every shift of every
 * window pair is screened on the first 64 bases of its overlap, the surviving (pair, shift) are verified over the whole overlap.
 * Limits (ISOCON_E_UNSUPPORTED): a shortest sequence of at most thr symbols (the reference's test is then true for degenerate reasons:
 * left to the host), thr > 1024, more than 0xfffffff0 window pairs or (pair, shift) survivors.  A store under its own map of at most
 * four symbols works unchanged (only equality matters); one with more than four symbols returns ISOCON_E_ALPHABET, with the message of
 * isocon_hw_pairs.  ISOCON_E_CAPACITY + *n_edges_needed when edges_cap is too small (out_row_ptr and the counters are valid then); the
 * number of window pairs bounds the edges.
 * out_counters (4 values, or NULL): window pairs, (pair, shift) survivors of the first-word test, pairs fully verified (those with a
 * survivor), invariant pairs (= edges).  *kernel_ms sums the window, screening, verification and row kernels.
 */
int isocon_end_invariant_graph(isocon_store *s, int32_t thr, uint64_t *out_row_ptr /* n + 1 */, uint32_t *out_cols, uint64_t edges_cap,
                               uint64_t *n_edges_needed, uint64_t *out_counters, float *kernel_ms);

/*
 * edlib.align(q, t, mode="NW", task="path", k) for a pair list (modules/edlib_alignment_module.py:130-135 edlib_traceback).
 * k NULL or k[p] < 0: unbounded.  out_ed[p] = distance, or -1 above k (then the pair has no ops).  Pair p owns
 * out_ops[out_ops_ptr[p] .. out_ops_ptr[p + 1]), len << 4 | code (0 '=', 1 'X', 2 'I' query only, 3 'D' target only), forward order,
 * adjacent ops differ, none empty.  Which optimal path is reported is the oracle's tie rule (from the end cell: 'I', then 'D', then the
 * diagonal; oracle/isocon_oracle.c orc_nw_path).  ISOCON_E_CAPACITY + *needed when ops_cap is too small (out_ed and out_ops_ptr are
 * valid then).
 * The distances come first, through the implementation of isocon_ed_pairs; only the pairs within their threshold are traced.  A path
 * of distance ed stays on at most ed + 1 diagonals (the corridor: |d| + 2 ((ed - |d|) / 2) + 1 of them, d = len_q - len_t).  A hit whose
 * corridor is at most 256 diagonals is traced by the banded kernels: one lane per pair, a window of 64, 128 or 256 rows that slides
 * along the corridor, 16 bytes of trace per column and 64 window rows -- 16 * len_t bytes at up to 64 diagonals, whatever len_q is.
 * Any other hit is traced by the un-banded kernel (one wavefront per pair, the whole query in 64-row blocks against the whole target,
 * 16 bytes of trace per block and column: about len_q * len_t / 4 bytes).  The traces of one launch of either kind stay within 1 GiB
 * of scratch: the list is cut into as many launches as that takes, and a single pair that needs more on its own is refused with
 * ISOCON_E_UNSUPPORTED (isocon_last_error states its sizes).  So is, among the hits of more than 256 diagonals only, a query of more
 * than 4 096 bases against a target of more than 655 360.  A pair with an empty sequence is answered
 * on the host (one 'D' or one 'I' op; none when both are empty).  A store under its own map of at most four symbols works unchanged
 * (only equality matters); one with more than four symbols returns ISOCON_E_ALPHABET; ids out of range ISOCON_E_ARG.
 * *kernel_ms sums the distance and the path kernels.
 */
int isocon_ed_path_pairs(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                         int32_t *out_ed, uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap, uint64_t *needed, float *kernel_ms);

/*
 * edlib.align(q, t, mode="HW", task="path", k) for a pair list: where inside the target the query sits and how it aligns there.
 * out (n_pairs, 5) holds exactly the rows of isocon_hw_pairs_wide for the same arguments (distance or -1, start, end, leading /
 * trailing insertion run), with that entry's checks and statuses: k[p] >= 0 required, k[p] > 2^20 ISOCON_E_UNSUPPORTED, ids out of
 * range ISOCON_E_ARG, a store of more than four symbols ISOCON_E_ALPHABET, an empty sequence a row of -1.  A pair with out[5 p] >= 0
 * owns out_ops[out_ops_ptr[p] .. out_ops_ptr[p + 1]), ops as in isocon_ed_path_pairs (len << 4 | code, 0 '=', 1 'X', 2 'I' query only,
 * 3 'D' target only; forward order, adjacent ops differ, none empty): the global alignment of the query against t[start..end] under the
 * oracle's tie rule (from the end cell: 'I', then 'D', then the diagonal; oracle.hw_path).  A pair above its threshold has no ops.
 * ISOCON_E_CAPACITY + *needed when ops_cap is too small (out and out_ops_ptr are valid then).
 * Two stages: the rows come through the implementation of isocon_hw_pairs_wide (banded kernels where the band fits), then every hit is
 * traced over its window alone by the kernels of isocon_ed_path_pairs: the banded ones where the corridor of (query, window, distance)
 * is at most 256 diagonals (16 bytes of trace per window column and 64 window rows), else the un-banded one (16 bytes per 64-row block
 * and window column); the target outside the window is not stored.  The traces of one launch stay within 1 GiB of scratch: the hits are
 * cut into as many launches as that takes, and a pair that needs more on its own is refused with ISOCON_E_UNSUPPORTED (isocon_last_error
 * states its sizes).  So is, among the hits of more than 256 diagonals only, a query of more than 4 096 bases against a window of more
 * than 655 360.  *kernel_ms sums both stages.
 */
int isocon_hw_path_pairs(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                         int32_t *out /* n_pairs x 5 */, uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap,
                         uint64_t *needed, float *kernel_ms);

/*
 * Every best location of an infix pair: the `locations` of edlib.align(q, t, mode="HW", task="path", k).  With D the infix matrix (zero
 * top row) of query q[p] (length P) and target t[p], h = min over columns j >= 1 of D[P][j]: out_ed[p] = h if h <= k[p], else -1.  A hit
 * owns the locations out_loc_ptr[p] .. out_loc_ptr[p + 1]), two int32 (start, end) each in out_locs: one per 0-based column end = j - 1 with
 * D[P][j] == h, in ascending order of the end, each with the smallest start s with ed(q, t[s..end]) == h.  The first location of a pair
 * is the (start, end) isocon_hw_pairs returns for it; a miss (out_ed[p] = -1: above k[p], an empty sequence, len(t) - len(q) < -k[p]) owns
 * none.  Argument checks, alphabet rule and band limit are those of isocon_hw_pairs: a store of more than four symbols ISOCON_E_ALPHABET, a
 * pair whose band max(len(t) - len(q), 0) + 2 k[p] + 1 exceeds 512 diagonals ISOCON_E_UNSUPPORTED for the call.  ISOCON_E_CAPACITY +
 * *needed when the locations exceed cap (out_ed and out_loc_ptr are valid then).  At most 2^32 - 16 locations per call.
 * All stages run on the device: the distance and first end of every pair by the kernels of isocon_hw_pairs, the ends by the same
 * recurrence on the hits with threshold h (run twice: count, then fill), the start of every (pair, end) by the start pass of
 * isocon_hw_pairs on diagonals [-h, h].  *kernel_ms sums them.
 */
int isocon_hw_locations(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                        int32_t *out_ed /* n_pairs */, uint64_t *out_loc_ptr /* n_pairs + 1 */, int32_t *out_locs /* cap x 2 */,
                        uint64_t cap, uint64_t *needed, float *kernel_ms);

/*
 * What the calling thread's last isocon_hw_locations call did (no counterpart in the reference; tests and timing scripts): out[0] pairs,
 * out[1] hits, out[2] locations, out[3] stages whose tiles were cut on the host (a run of 64 pairs of one query with a common window
 * above 512 diagonals), then the tiles per class of 1, 2, 4, 8 window words of the distance stage out[4..7], of an ends run out[8..11]
 * and of the start stage out[12..15].  Writes min(cap, 16) values and returns that number.
 */
int isocon_hw_locations_last_stats(double *out, int32_t cap);

/*
 * isocon_hw_locations without the limit of 512 diagonals: the same arguments, outputs in the caller's pair order, semantics and capacity
 * protocol (ISOCON_E_CAPACITY + *needed with out_ed and out_loc_ptr valid and out_locs untouched), with the checks and limits of
 * isocon_hw_pairs_wide: ids out of range or k[p] < 0 ISOCON_E_ARG, k[p] > 2^20 ISOCON_E_UNSUPPORTED, a store of more than four symbols
 * ISOCON_E_ALPHABET, a query of more than 4 096 bases against a target of more than 655 360 ISOCON_E_UNSUPPORTED (before any launch);
 * len(t) - len(q) < -k[p] is a miss.  Nothing is traced, so no pair is refused for its size otherwise.  The first location of a hit is
 * the (start, end) of isocon_hw_pairs_wide.
 * Every pair is classed on the host from the two lengths and k[p] as isocon_hw_pairs_wide classes it: the pairs whose own band fits go
 * through the implementation of isocon_hw_locations as one sub-list in their order (a call without any other pair IS that call), the
 * others through un-banded kernels that run the recurrence twice and keep nothing per column: a count run (distance, first end, number
 * of ends; an exclusive scan of the counts gives the row pointers) and a fill run that lists the ends.  A query of at most 256 bases
 * takes one LANE of a kernel that holds the whole query in registers (1, 2 or 4 words of 64 rows), a longer one a wavefront (64 rows
 * per lane).  The start of an end with distance h <= 255 comes from the start pass of isocon_hw_locations on diagonals [-h, h], that of
 * an end with a larger distance from an un-banded start pass, one wavefront per end.  *kernel_ms sums all of it.
 */
int isocon_hw_locations_wide(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                             int32_t *out_ed /* n_pairs */, uint64_t *out_loc_ptr /* n_pairs + 1 */, int32_t *out_locs /* cap x 2 */,
                             uint64_t cap, uint64_t *needed, float *kernel_ms);

/*
 * What the calling thread's last isocon_hw_locations_wide call did (no counterpart in the reference; tests and timing scripts): out[0]
 * pairs, out[1] pairs that went through isocon_hw_locations, out[2] wide pairs, out[3] hits, out[4] locations (both of all pairs),
 * out[5..7] wide pairs on the lane-per-pair kernel with 1, 2, 4 query words, out[8] wide pairs on the wavefront-per-pair kernel,
 * out[9] (pair, end) entries of wide pairs whose start came from the banded start pass, out[10] from the un-banded one, out[11]
 * launches for the wide pairs (0 when the call had none), out[12] kernel milliseconds.  Writes min(cap, 13) values and returns that
 * number.
 */
int isocon_hw_locations_wide_last_stats(double *out, int32_t cap);

/*
 * Prefix alignments of a pair list: edlib.align(q, t, mode="SHW", k) -- the whole query against a PREFIX of the target (a primer that
 * must sit at the read's start; on reversed strings, at its end).  With D the global matrix of query q[p] (length P) and target t[p]
 * (length n) -- D[0][j] = j, D[i][0] = i -- h = min over columns 1 <= j <= n of D[P][j] = min over j of ed(q, t[0..j)): out_ed[p] = h if
 * h <= k[p], else -1.  A hit owns the ends out_ends[out_end_ptr[p] .. out_end_ptr[p + 1]): every 0-based column end = j - 1 with
 * D[P][j] == h, ascending; they lie in [P - h - 1, P + h - 1], at most 2 h + 1 of them, and edlib's `locations` are (0, end) for each.
 * A miss (above k[p], an empty sequence, n - P < -k[p]) owns none.  k[p] >= 0 is required (ISOCON_E_ARG, as an id out of range); a
 * threshold above len(q) asks no more than len(q) (h <= P) and is taken as that.  A store of more than four symbols returns
 * ISOCON_E_ALPHABET.  ISOCON_E_CAPACITY + *needed when the ends exceed cap (out_ed and out_end_ptr are valid then).  At most 2^32 - 16
 * pairs and ends per call.
 * All stages run on the device, on a band of 2 thr + 1 diagonals whatever the target's length is (only its first P + thr columns are
 * read).  The distance stage runs in up to four rounds of thresholds min(k[p], 31), 63, 127, 255 -- windows of 1, 2, 4, 8 words --; a
 * pair leaves them when it hits or has missed at its own threshold, so an unbounded search costs what its distance needs.  A pair
 * that no round settles (k[p] > 255 and h > 255; never a query of at most 255 bases) fails the call with ISOCON_E_UNSUPPORTED, and
 * isocon_last_error names the first such pair: there is no un-banded prefix pass.  The ends come from the same recurrence on the hits
 * with threshold h, run twice (count, then fill).  *kernel_ms sums the stages.
 */
int isocon_shw_locations(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                         int32_t *out_ed /* n_pairs */, uint64_t *out_end_ptr /* n_pairs + 1 */, int32_t *out_ends /* cap */,
                         uint64_t cap, uint64_t *needed, float *kernel_ms);

/*
 * edlib.align(q, t, mode="SHW", task="path", k) for a pair list.  out (n_pairs, 2) = (distance or -1, first end or -1) of
 * isocon_shw_locations for the same arguments, with that entry's checks, statuses and rounds.  A hit owns
 * out_ops[out_ops_ptr[p] .. out_ops_ptr[p + 1]), ops as in isocon_ed_path_pairs: the global alignment of the query against
 * t[0 .. end] for the FIRST end, under the tie rule used everywhere else (from the end cell: 'I', then 'D', then the diagonal); a miss
 * has no ops.  ISOCON_E_CAPACITY + *needed when ops_cap is too small (out and out_ops_ptr are valid then).  The paths come from the
 * trace kernels of isocon_ed_path_pairs over the window of end + 1 columns (isocon_path_last_stats tells their classes).
 */
int isocon_shw_path_pairs(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                          int32_t *out /* n_pairs x 2 */, uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap,
                          uint64_t *needed, float *kernel_ms);

/*
 * What the calling thread's last isocon_shw_locations / isocon_shw_path_pairs call did (no counterpart in the reference; tests and
 * timing scripts): out[0] pairs, out[1] hits, out[2] ends (locations entry only), out[3] rounds of the distance stage that ran,
 * out[4..7] pairs entering round 0 .. 3, out[8..11] tiles of the distance stage per class of 1, 2, 4, 8 window words summed over the
 * rounds, out[12..15] tiles of an ends run per class.  Writes min(cap, 16) values and returns that number.
 */
int isocon_shw_last_stats(double *out, int32_t cap);

/*
 * How the calling thread's last isocon_ed_path_pairs / isocon_hw_path_pairs call traced its hits (no counterpart in the reference).
 * out[0] hits traced; out[1..3] hits of the banded classes of 1, 2 and 4 window words (64, 128, 256 diagonals); out[4] hits of the
 * un-banded kernel; out[5] / out[6] bytes of trace banded / un-banded; out[7] / out[8] launches banded / un-banded; out[9] / out[10]
 * kernel milliseconds of the banded trace + walk / the un-banded one; out[11] of the forward-op kernel.  Either entry zeroes the values
 * when it is called: a call without pairs or hits, and one that fails before its hits are classed or refuses one of them
 * (ISOCON_E_ARG, ISOCON_E_ALPHABET, a failure of the distance or row stage, ISOCON_E_UNSUPPORTED), reports zeros; one that fails later
 * (ISOCON_E_CAPACITY) reports what it had done.  Writes min(cap, 12) values and returns that number.
 */
int isocon_path_last_stats(double *out, int32_t cap);

/*
 * Device read tables of the hypothesis test: which reads support a candidate against its reference, and every read's error counts,
 * from the stored read alignments -- the per-read loops of get_support (modules/functions.py:149-201), get_read_errors (:204-216) and
 * read_errors_from_alignment (:495-522) as arrange_alignments_new_no_realign calls them per edge (modules/hypothesis_test_module.py:92-171).
 * Integers and bit sets, and with base qualities the reads' error probabilities (isocon_readtab_probability); the p-value stays on the host.
 *
 * A table set holds the alignments of the reads of many candidates.  Row r is the pair of gapped rows (candidate's, read's)
 * ref_rows / read_rows[row_ptr[r] .. row_ptr[r + 1]) (one row_ptr: both rows of an alignment are equally long), table k = rows
 * first_row[k] .. first_row[k + 1] = the reads of one candidate (first_row[0] = 0, first_row[n_tables] = n_rows).
 *   isocon_readtab_create        uploads the rows, builds the tables (k_rt_build) and returns out_errors[3 r ..] = (insertions, deletions,
 *                                substitutions) of row r between the end gaps of either row == read_errors_from_alignment.
 *                                ISOCON_E_ARG: a byte outside ACGT-, offsets that descend, rows of one table with different numbers of
 *                                candidate bases.  The handle keeps, per row and 64-column block, the mask of columns without a
 *                                candidate base, the mask of differing columns and the count of candidate bases before the block, and
 *                                the reads' bytes; the candidates' bytes are not kept.
 *   isocon_readtab_support       query q = one side of one edge: table q_table[q], kind q_kind[q], its variants var_ptr[q] .. var_ptr[q + 1]
 *                                in the dict order of get_variant_coordinates (:89-146): var_pos = coordinate i on the candidate, var_u
 *                                = u_v, var_type = the type letter ('I', 'D', 'S').  Bit j of out_bits[bits_ptr[q] + j / 64] = row j of
 *                                the table passes every variant; out_count[q] = their number; the caller sizes the bit set
 *                                (bits_ptr[q + 1] - bits_ptr[q] >= ceil(rows / 64), bits_ptr[0] = 0; spare words come back 0).
 *                                  kind 0 (reads of c): pos = column of candidate base i of the row; passes iff no column of
 *                                    [pos - 1, pos + u_v] inside the row differs between the two rows (:186-190).
 *                                  kind 1 (reads of t): (before, after) = (2, u_v) for 'I', else (1, u_v + 1); passes iff
 *                                    read_row[max(0, pos - before) .. min(len, pos + after)) equals the variant's snippet
 *                                    snip_bytes[snip_ptr[v] .. snip_ptr[v + 1]) (v = index into the variant arrays), length included
 *                                    (:192-199).  snip_ptr / snip_bytes may be NULL when no query of kind 1 has a variant.
 *                                i in [-ref_len, 0) counts from the end as a Python index does; any other i outside [0, ref_len) is
 *                                ISOCON_E_ARG (the per-read statement raises IndexError) unless the table has no rows.  u_v and the
 *                                snippet length are not limited by the block size.
 *   isocon_readtab_set_qualities attaches base qualities (FASTQ input) to the table set: row r owns the record qual[qual_ptr[r] ..
 *                                qual_ptr[r + 1]) (its length is rec_len), the read of row r starts at rec_start[r] in it (CCS.seq.index,
 *                                modules/ccs_info.py:37-56).  Uploads them and fills, per row and 64-column block, the mask of gap columns
 *                                of the read's row and the count of read bases before the block (k_rt_read_prefix).  These buffers exist
 *                                only after this call; a second call replaces the first.  ISOCON_E_ARG: a quality above 93, offsets
 *                                that descend (the handle keeps what it had).
 *   isocon_readtab_quality       the queries of isocon_readtab_support (same arrays, same wrapping and refusal of coordinates; snippets
 *                                for BOTH kinds) answered with one byte per (variant, row): out_codes[code_ptr[q] + v rows + j] for the
 *                                v-th variant of query q and row j of its table; the caller sizes the range (code_ptr[q + 1] -
 *                                code_ptr[q] >= variants x rows, code_ptr[0] = 0; spare bytes come back 0).  The byte restates
 *                                get_read_ccs_probabilities_c / _t (modules/functions.py:240-331 kind 0, :334-433 kind 1) up to the
 *                                quality they look up.  pos = column of candidate base i; shows_own = no differing column in
 *                                [pos - 1, pos + u_v]; shows_other = the window of isocon_readtab_support's kind 1 equals the snippet,
 *                                "insertion style" (2 before, u_v after) when the type is 'D' (kind 0) / 'I' (kind 1); seen = read
 *                                bases in the read's row up to and including pos; read_coord = seen - 1 if shows_own, else seen + off
 *                                with off = 0 for 'I' and -1 otherwise (kind 0), 0 for 'D', -2 for 'I' and -1 otherwise (kind 1);
 *                                coord = rec_start + read_coord, then as CCS.read_aln_to_ccs_coord and a Python list index do:
 *                                coord > rec_len is "beyond", coord == rec_len takes coord - 1, coord < 0 takes coord + rec_len, a
 *                                result outside [0, rec_len) is "index".
 *                                  0 .. 93  the quality at coord          0xFF  neither row is shown (the read is not informative)
 *                                  0xFE     both are shown                0xFD  beyond the record (the reference exits)
 *                                  0xFC     index out of range (the reference raises IndexError)
 *                                both > neither > beyond > index > quality.  A byte depends on its own (variant, row) only: dropping a
 *                                read at an earlier variant, and raising for a read that is still informative, is the caller's.
 *                                ISOCON_E_ARG: no qualities attached.
 *   isocon_readtab_probability   the queries of isocon_readtab_quality (the very arrays, snippets for both kinds, the same checks) answered
 *                                with one double per row: what the variant loop of get_read_ccs_probabilities_c / _t
 *                                (modules/functions.py:240-433) multiplies up for that read, so the code bytes never leave the device.
 *                                q_ratios[3 q ..] = the (substitution, insertion, deletion) shares of the errors of query q's edge,
 *                                p_of_quality[0 .. 93] = the error probability of every quality value.  A row starts informative with
 *                                p = 1.0 and takes the query's variants in order; at a variant with code byte
 *                                  0xFF       it stops being informative: its answer is -1.0, later variants do nothing to it;
 *                                  0xFE / 0xFD / 0xFC  (while informative) it raises: its answer is -2.0, later variants do nothing;
 *                                  0 .. 93    p = p * p_error with p10 = p_of_quality[code] and p_error = p10 if u_v > 1, else
 *                                             (p10 * substitution share) / 3.0 for 'S', (p10 * insertion share) / 4.0 for 'I',
 *                                             p10 * deletion share for any other type (:305-320, :406-421)
 *                                in IEEE binary64, each product and quotient rounded once, in exactly that association: equal to the
 *                                host's doubles in every bit, subnormal and zero products included (whether 0 < p < 1 holds is the
 *                                caller's to assert).  out_prob[prob_ptr[q] + j] = row j of query q's table; the caller sizes the range
 *                                (prob_ptr[q + 1] - prob_ptr[q] >= rows, prob_ptr[0] = 0; spare slots come back 0.0); a query without
 *                                variants answers 1.0 for every row.  out_status[q] = 0 if no row of the query raised, else
 *                                ((v + 1) << 8) | code byte of what the per-read statements meet first: the smallest variant index v
 *                                (0-based in the query) at which an informative row raises, and among the rows at that variant both
 *                                (0xFE, an assertion) before beyond (0xFD, an exit) before index (0xFC, IndexError).  The answers of
 *                                a query with a non-zero status are not the reference's: it raises there.  ISOCON_E_ARG: no qualities
 *                                attached; q_ratios, p_of_quality, prob_ptr or out_status NULL; more than 2^24 - 2 variants in a query;
 *                                and whatever isocon_readtab_quality refuses.
 *   isocon_readtab_device_bytes  device memory the handle holds (the qualities' buffers included).
 */
typedef struct isocon_readtab isocon_readtab;
int isocon_readtab_create(const uint8_t *ref_rows, const uint8_t *read_rows, const uint64_t *row_ptr, uint32_t n_rows, const uint32_t *first_row,
                          uint32_t n_tables, isocon_readtab **out, uint32_t *out_errors, float *kernel_ms);
int isocon_readtab_support(isocon_readtab *h, uint32_t n_queries, const uint32_t *q_table, const uint8_t *q_kind, const uint64_t *var_ptr,
                           const int32_t *var_pos, const int32_t *var_u, const uint8_t *var_type, const uint64_t *snip_ptr, const uint8_t *snip_bytes,
                           const uint64_t *bits_ptr, uint64_t *out_bits, uint32_t *out_count, float *kernel_ms);
int isocon_readtab_set_qualities(isocon_readtab *h, const uint8_t *qual, const uint64_t *qual_ptr, const uint32_t *rec_start, float *kernel_ms);
int isocon_readtab_quality(isocon_readtab *h, uint32_t n_queries, const uint32_t *q_table, const uint8_t *q_kind, const uint64_t *var_ptr,
                           const int32_t *var_pos, const int32_t *var_u, const uint8_t *var_type, const uint64_t *snip_ptr, const uint8_t *snip_bytes,
                           const uint64_t *code_ptr, uint8_t *out_codes, float *kernel_ms);
int isocon_readtab_probability(isocon_readtab *h, uint32_t n_queries, const uint32_t *q_table, const uint8_t *q_kind, const uint64_t *var_ptr,
                               const int32_t *var_pos, const int32_t *var_u, const uint8_t *var_type, const uint64_t *snip_ptr, const uint8_t *snip_bytes,
                               const double *q_ratios /* 3 per query: substitution, insertion, deletion */, const double *p_of_quality /* 94 */,
                               const uint64_t *prob_ptr, double *out_prob, uint32_t *out_status, float *kernel_ms);
void isocon_readtab_destroy(isocon_readtab *h);
uint64_t isocon_readtab_device_bytes(const isocon_readtab *h);

/*
 * The variants of candidate-vs-reference edges of the hypothesis test from the alignments' CIGAR ops: what _candidate_vs_reference
 * (modules/hypothesis_test_module.py:99-110), get_mask_start_and_end (modules/functions.py:218-236) and get_variant_coordinates (:89-146)
 * compute on the two gapped strings of an alignment -- which never exist here (kernels: isocon_amd/csrc/edgevar.hpp).  Independent of a
 * store: sequence s = seqs[seq_ptr[s] .. seq_ptr[s + 1]) (ASCII, ACGT; at most 2^30 bases), edge e = (reference edge_t[e], candidate edge_c[e]),
 * both ids into seqs.  Its two alignments in isocon_sg_trace_batch's encoding: list 2 e = ops[ops_ptr[2 e] .. ops_ptr[2 e + 1]) aligns (t, c)
 * (t is the query), list 2 e + 1 aligns (c, t).  The variants are the columns of ops other than '=' outside the leading and trailing gap run
 * of either row ('=' against 'X' is trusted); the (c, t) list replaces the (t, c) one only with strictly fewer variants (out_flipped[e] = 1).
 * The caller gives edge e the record slots rec_ptr[e] .. rec_ptr[e + 1) -- enough is the larger of its two lists' summed lengths of ops other
 * than '=' -- and gets out_n_var[e] records of 8 int32 in out_recs[8 s ..], in column order:
 *     column i, t_last, c_last (bases of t / c in aln[:i + 1], minus one), key on t, key on c ('D': t_last, c_last + 1; 'I': t_last + 1,
 *     c_last; 'S': t_last, c_last), u_v, snippet length, type letter | p_t << 8 | p_c << 16 (the two rows' characters in column i)
 * Every variant is there: filing them under their keys in this order gives the reference's dicts, overwritten entries and key order
 * included.  Spare slots come back 0.  out_snip_ptr has rec_ptr[n_edges] - rec_ptr[0] + 1 entries: the snippets aln_c / aln_t[max(0, i - 1)
 * : i + u_v + 1] of slot s are out_snip_c / out_snip_t[out_snip_ptr[s] .. out_snip_ptr[s + 1]).  The caller sizes the two byte buffers
 * (snip_cap each); *n_snip_needed always returns the size needed, and ISOCON_E_CAPACITY means that everything but the snippet bytes is
 * valid and the call has to be repeated with larger buffers.
 * out_bad[e] = 1, and no record, for an edge one of whose lists does not consume exactly len(t) and len(c), uses a code above 3 or holds
 * an op of length 0.  ISOCON_E_ARG (isocon_last_error names the first such edge): an id out of range, an empty sequence, offsets that
 * descend, more variants than the edge's slots.  ISOCON_E_ALPHABET: a byte outside ACGT.  n_edges = 0 is ISOCON_OK.
 */
int isocon_edge_variants(const uint8_t *seqs, const uint64_t *seq_ptr, uint32_t n_seqs, uint32_t n_edges, const uint32_t *edge_t, const uint32_t *edge_c,
                         const uint32_t *ops, const uint64_t *ops_ptr, const uint64_t *rec_ptr, uint8_t *out_flipped, uint32_t *out_n_var, uint8_t *out_bad,
                         int32_t *out_recs, uint64_t *out_snip_ptr, uint8_t *out_snip_c, uint8_t *out_snip_t, uint64_t snip_cap, uint64_t *n_snip_needed,
                         float *kernel_ms);

/*
 * Raghavan's bound of hypothesis_test_module.py:253-329 for n tests: from m_sum[i] = E[Y] and y_sum[i] = the summed weights of the
 * supporting reads the reference evaluates, in 100-digit decimals, d = y / m - 1, k = m d and e^k / (1 + d)^(k + k / d) and returns float()
 * of it; y == 0 gives 1.0 and d == 0 gives 0.5.  As 1 + d = y / m, k = y - m and k / d = m, that is f = exp((y - m) - y (ln y - ln m)).  A lane
 * evaluates f in 320-bit fixed point with a bound on its own error, to which the deviation of the reference's decimals from f (below 10^-89
 * relative inside the domain) is added, and rounds to a double only where the discarded bits are farther from the halfway pattern than 2^22
 * times that bound (kernel: isocon_amd/csrc/pbound.hpp, derivation: DESIGN.md 4.7).
 *   out_certified[i] = 1: out_bound[i] has the bits of float() of the reference's 100-digit result.
 *   out_certified[i] = 0: out_bound[i] comes back 0.0 and the caller evaluates the test itself (the reference statement then returns or
 *                         raises what it always did).
 * Certified domain: m and y finite, normal, positive and below 2^31, y |ln(y / m)| and |y - m| below floor(9 10^5 ln 10) = 2072326 (beyond
 * y |log10(y / m)| = |y - m| log10(e) = 9 10^5 the decimals overflow or lose digits), and the exponent of y at most 300 below that of m (y / m >
 * 2^-301: the reference's 1 + d keeps 100 - log10(m / y) digits of y / m, and below y / m = 5 10^-101 it is 0 and the reference raises).  Special cases, decided on the doubles' bits for such an
 * m: y == +0.0 -> 1.0, y == m -> 0.5, both certified.  NaN, infinities, negative numbers (-0.0 too), m == 0 and subnormal inputs are never certified.
 * No store, no handle.  n = 0 is ISOCON_OK; a NULL array with n > 0, or n > 2^32, ISOCON_E_ARG; no device ISOCON_E_NODEVICE.  Only the first n
 * entries of the two outputs are written.
 */
int isocon_raghavan_bound(const double *m_sum, const double *y_sum, uint64_t n, double *out_bound, uint8_t *out_certified, float *kernel_ms);

/*
 * Greedy partition of the nearest-neighbour graph into consensus centres and their members, on integer ids: what
 * get_partitions_no_copy (modules/partitions.py:301-413, called by partition_strings :416-593 on nx.reverse(G_star)) and
 * partition_highest_reachable_with_edge_degrees (modules/end_invariant_functions.py:405-533; nbr_tiebreak = 0) compute on networkx
 * graphs keyed by the sequences.  Host-only (no GPU work): the graph is the edge list the NN search returns.
 *   n nodes, degree[i] = multiplicity of sequence i (graphs.py:37-51), edges (edge_a[e] -> edge_b[e]): b is a nearest neighbour of a
 *   (an edge of G*), rank[i] = position of sequence i in the lexicographic order of the sequences (the reference breaks ties with
 *   `m < centre` on the strings), nbr_tiebreak != 0: between start nodes of equal reachable weight prefer more direct in-neighbours.
 * Output, in the reference's extraction order (components by size, largest first): out_centre[p], out_weight[p] = total multiplicity
 * of partition p, its other members out_members[out_member_ptr[p] .. out_member_ptr[p + 1]) (any order: the reference returns sets).
 * Capacities: out_centre / out_weight n entries, out_member_ptr n + 1, out_members n.  Deterministic where the reference depends on
 * PYTHONHASHSEED (ties between different reachable sets of equal weight: SURVEY.md F6).
 */
int isocon_partition_ids(uint32_t n, const int32_t *degree, uint64_t n_edges, const uint32_t *edge_a, const uint32_t *edge_b,
                         const uint32_t *rank, int32_t nbr_tiebreak, uint32_t *out_centre, int64_t *out_weight,
                         uint64_t *out_member_ptr, uint32_t *out_members, uint32_t *n_parts);

#ifdef __cplusplus
}
#endif
#endif
