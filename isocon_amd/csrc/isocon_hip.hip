// isocon_hip.hip -- C ABI of libisocon_hip.so (see include/isocon_hip.h).  Host orchestration + kernel launches.
// gfx950 only.  One process drives one GPU (isocon_init selects it).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "ed_band.hpp"
#include "ed_full.hpp"
#include "qgram_mm.hpp"
#include "nn.hpp"
#include "nn_list.hpp"
#include "nn_filter.hpp"
#include "nn_finalize.hpp"
#include "nn_finalize_host.hpp"
#include "partition_host.hpp"
#include "ed_pairs_plan.hpp"
#include "sg.hpp"
#include "msa.hpp"
#include "hw.hpp"
#include "hw_tiles.hpp"
#include "hw_plan.hpp"
#include "nwp_plan.hpp"
#include "hw_loc.hpp"
#include "shw.hpp"
#include "hw_full.hpp"
#include "hw_rows.hpp"
#include "hw_graph.hpp"
#include "end_inv.hpp"
#include "nw_path.hpp"
#include "nw_band.hpp"
#include "ed_lanes.hpp"
#include "ed_bytes.hpp"
#include "nn2_depth.hpp"
#include "readtab.hpp"
#include "edgevar.hpp"
#include "pbound.hpp"

namespace isocon {
thread_local std::string g_last_error;
}

using namespace isocon;

// ISOCON_DEBUG_VARIANT = "name[=value],name,...": the ONE environment switch behind which every diagnostic / A-B variant of the kernel
// selection sits (tests force fallbacks and superseded paths through it; DESIGN.md section 8 lists the names).  Unset -- production -- every
// input class has one code path.  variant(name): the name is listed; variant_value(name): its value ("" if listed without one), nullptr if
// not listed (the pointer is good until eight further calls on this thread).
static bool variant_lookup(const char *name, std::string *value)
{
    const char *e = getenv("ISOCON_DEBUG_VARIANT");
    if (!e) return false;
    const size_t ln = strlen(name);
    for (const char *p = e; *p;) {
        const char *q = strchr(p, ',');
        const size_t len = q ? (size_t)(q - p) : strlen(p);
        if (len >= ln && strncmp(p, name, ln) == 0 && (len == ln || p[ln] == '=')) {
            if (value) *value = len > ln ? std::string(p + ln + 1, len - ln - 1) : std::string();
            return true;
        }
        p += len + (q ? 1 : 0);
    }
    return false;
}
static bool variant(const char *name) { return variant_lookup(name, nullptr); }
static const char *variant_value(const char *name)
{
    thread_local std::string ring[8];
    thread_local unsigned at = 0;
    std::string &slot = ring[at++ % 8];
    return variant_lookup(name, &slot) ? slot.c_str() : nullptr;
}

// What the pool's nearest-neighbour slots currently hold, next to the slots themselves (no free-floating state: a store reaches it
// through its pool, and whoever overwrites or releases a slot invalidates the tag in the same place).
// BoundTag: the q-gram bound matrix of the last seed phase (slot SLOT_NN_LB; its row offsets and row lengths inside SLOT_NN_LBCHUNKS, where
// lb_row and lb_len point): the main phase of the SAME store and shard that follows uses it instead of computing it again.  Identified
// by the store's serial number (not its address).
struct BoundTag {
    bool valid = false, has_order = false;
    uint64_t serial = 0;
    QMap map = {0, 0, 0, 0};
    uint32_t depth = 0;
    int32_t kcap = 0;
    unsigned long long lb_total = 0;
    const unsigned long long *lb_row = nullptr;
    const uint32_t *lb_len = nullptr;
};
// MsaBuilt: the matrices a build left in SLOT_MSA_IN (their partition tables in SLOT_MSA_PART .. SLOT_MSA_CBASE) for the correction that
// follows, with the host's copy of their layout.  `by`: which entry point built them -- isocon_msa_correct_built / isocon_msa_read_built pair
// with isocon_msa_build_ops only, isocon_msa_correct_built_batch with isocon_msa_build_ops_batch only.
struct MsaBuilt {
    enum By { NONE, SINGLE, BATCH } by = NONE;
    uint64_t serial = 0;
    uint32_t n_parts = 0, n_rows = 0;
    std::vector<uint32_t> ncols, col_base, first_row;
    std::vector<unsigned long long> m_off;
};
// HeldHits: candidate edges of a sharded search that stay in device memory from phase to phase (SLOT_NN_ACC_HITS), tagged with their store.
struct HeldHits { uint64_t store_serial = 0; uint64_t rows = 0; };

// Grow-only device scratch owned by the store: repeated calls reuse their buffers instead of paying
// hipMalloc/hipFree (tens of ms for the multi-GB trace scratch) every time.
struct ScratchPool {
    struct Slot { void *p = nullptr; size_t cap = 0; };
    Slot slots[208];
    BoundTag bound_tag;
    HeldHits held_hits;
    MsaBuilt msa;
    void *get(int idx, size_t bytes)
    {
        Slot &s = slots[idx];
        if (bytes == 0) bytes = 16;
        if (s.cap < bytes) {
            if (s.p) (void)hipFree(s.p);
            s.p = nullptr; s.cap = 0;
            const size_t want = bytes + bytes / 8;
            if (hipMalloc(&s.p, want) == hipSuccess) s.cap = want;
            else if (hipMalloc(&s.p, bytes) == hipSuccess) s.cap = bytes;
            else { s.p = nullptr; (void)hipGetLastError(); }
        }
        return s.p;
    }
    void release()
    {
        for (Slot &s : slots) { if (s.p) (void)hipFree(s.p); s.p = nullptr; s.cap = 0; }
        bound_tag = BoundTag();
        held_hits = HeldHits();
        msa = MsaBuilt();
    }
};

enum {
    SLOT_ED_TS = 0, SLOT_ED_IDS, SLOT_ED_K, SLOT_ED_OUT, SLOT_FULL_A, SLOT_FULL_B, SLOT_FULL_K, SLOT_FULL_OUT,
    SLOT_NN_BEST, SLOT_NN_QF, SLOT_NN_TF, SLOT_NN_HITS, SLOT_NN_HITCOUNT, SLOT_NN_STATS, SLOT_NN_TS, SLOT_NN_IDS, SLOT_NN_PLANES2, SLOT_NN_PERM, SLOT_NN_IL, SLOT_NN_IL2, SLOT_NN_HITS2, SLOT_NN_HITCOUNT2, SLOT_NN_QPROF, SLOT_NN_QSUM, SLOT_NN_LB, SLOT_NN_SLOTORDER, SLOT_NN_LBCHUNKS, SLOT_NN_ROWMIN, SLOT_NN_COLMIN, SLOT_NN_SEED_A, SLOT_NN_SEED_B, SLOT_NN_SEED_N, SLOT_NN_LBT, SLOT_NN_LBT_OFF, SLOT_NN_LBT_SLO, SLOT_NN_LBT_LEN, SLOT_NN_LBT_PAD, SLOT_NN_SCORE, SLOT_NN_LDEST, SLOT_NN_FIN_HITS, SLOT_NN_FIN_CNT, SLOT_NN_FIN_START, SLOT_NN_FIN_CUR, SLOT_NN_FIN_NB, SLOT_NN_FIN_LEN2, SLOT_NN_FIN_OUT, SLOT_NN_FIN_FLAG, SLOT_NN_FIN_BEST, SLOT_NN_ACC_HITS, SLOT_NN_LTOT, SLOT_NN_LCHUNKS, SLOT_NN_LIST, SLOT_NN_LPA, SLOT_NN_LPB, SLOT_NN_TEXT2, SLOT_NN_LTASKS, SLOT_NN_RECORD, SLOT_NN_SEED_KNOWN,
    SLOT_NN2_STATE, SLOT_NN2_TPOS, SLOT_NN2_EXC, SLOT_NN2_CTR, SLOT_NN2_PAIRS, SLOT_NN2_WIDE,
    SLOT_SG_PAIRS, SLOT_SG_R, SLOT_SG_TRACE, SLOT_SG_END, SLOT_SG_OPS, SLOT_SG_CNT, SLOT_SG_RES, SLOT_SG_OFF, SLOT_SG_DENSE, SLOT_SG_BOUND, SLOT_SG_AOFF, SLOT_SG_ALNA, SLOT_SG_ALNB,
    SLOT_MSA_IN, SLOT_MSA_OUT, SLOT_MSA_DEG, SLOT_MSA_COUNTS, SLOT_MSA_MAJ, SLOT_MSA_FLAGS, SLOT_MSA_TOT, SLOT_MSA_NCAND, SLOT_MSA_LEN, SLOT_MSA_OFF, SLOT_MSA_PACKED, SLOT_MSA_ROWS, SLOT_MSA_OPS, SLOT_MSA_OPTR, SLOT_MSA_LONGEST, SLOT_MSA_WIDTH, SLOT_MSA_CSLOT, SLOT_MSA_LTOT, SLOT_MSA_WIDE, SLOT_MSA_PROW, SLOT_MSA_PCOL, SLOT_MSA_PPTR, SLOT_MSA_PBYTES, SLOT_MSA_PART, SLOT_MSA_FIRST, SLOT_MSA_LM, SLOT_MSA_SBASE, SLOT_MSA_NCOLS, SLOT_MSA_MOFF, SLOT_MSA_CBASE, SLOT_MSA_CBP, SLOT_MSA_CBC, SLOT_MSA_CBR, SLOT_MSA_WIDX, SLOT_MSA_KEYS, SLOT_MSA_LEFT,
    SLOT_HW_Q, SLOT_HW_T, SLOT_HW_K, SLOT_HW_OUT, SLOT_HW_TRACE, SLOT_HW_CTR, SLOT_HW_TILEQ, SLOT_HW_LANES, SLOT_HW_PQ, SLOT_HW_KEY, SLOT_HW_HIST, SLOT_HW_CURSOR, SLOT_HW_TBASE, SLOT_HW_CLS,
    SLOT_HWL_THR, SLOT_HWL_CNT, SLOT_HWL_PTR, SLOT_HWL_EQ, SLOT_HWL_ET, SLOT_HWL_EH, SLOT_HWL_EHE, SLOT_HWL_LOCS, SLOT_SHW_ENTER,
    SLOT_HWLW_Q, SLOT_HWLW_T, SLOT_HWLW_K, SLOT_HWLW_HE, SLOT_HWLW_CNT, SLOT_HWLW_PTR, SLOT_HWLW_LIST, SLOT_HWLW_ULIST, SLOT_HWLW_FLAGS,
    SLOT_HWG_CD, SLOT_HWG_TOT, SLOT_HWG_FIRST, SLOT_HWG_CTR, SLOT_HWG_VALUE, SLOT_HWG_ROWCNT, SLOT_HWG_ROWPTR, SLOT_HWG_COLS, SLOT_HWG_ED,
    SLOT_EINV_LO, SLOT_EINV_TOT, SLOT_EINV_FIRST, SLOT_EINV_CTR, SLOT_EINV_BEST, SLOT_EINV_SURV, SLOT_EINV_ROWCNT, SLOT_EINV_ROWPTR, SLOT_EINV_COLS,
    SLOT_PACK_ASCII, SLOT_PACK_OFF, SLOT_PACK_BAD, SLOT_PACK_HIST, SLOT_PACK_FLAGS, SLOT_EB_A, SLOT_EB_B, SLOT_EB_K, SLOT_EB_OUT, SLOT_EB_ROWS, SLOT_SCAN_TMP, SLOT_SCAN_SUMS, SLOT_SCAN_TMP_SIDE, SLOT_SCAN_SUMS_SIDE,
    SLOT_RT_REF, SLOT_RT_IN, SLOT_RT_OUT,
    SLOT_EV_IN, SLOT_EV_OUT, SLOT_EV_SNIP,
    SLOT_PB_IN, SLOT_PB_OUT,
    SLOT_NWP_Q, SLOT_NWP_T, SLOT_NWP_ED, SLOT_NWP_TOFF, SLOT_NWP_ROFF, SLOT_NWP_REV, SLOT_NWP_RUNS, SLOT_NWP_FOFF, SLOT_NWP_OPS, SLOT_NWP_START, SLOT_NWP_COLS,
    SLOT_NWB_TRACE, SLOT_NWB_SLOTS, SLOT_NWB_WOFF, SLOT_NWB_WCOLS, SLOT_NWB_WLANES,
    SLOT_COUNT
};
static_assert(SLOT_COUNT <= 208, "ScratchPool::slots too small");

// One pool per process (one process drives one GPU): scratch outlives the individual stores, because the Python
// wrappers create a fresh store per call (the reference's functions are stateless).
static ScratchPool g_scratch;

static uint64_t g_store_serial = 0;

struct isocon_store {
    uint64_t serial = ++g_store_serial;
    DevStore dev;
    // isocon_store_create_ptrs_ex(..., ISOCON_STORE_PRIVATE_SCRATCH): the store gets a scratch pool of its own, released with it --
    // for runs that emulate SEVERAL ranks inside one process (tests/baton_dist.py): a rank's bound matrix, held candidate edges and
    // counters must not be another rank's.  A real rank is a process, and its stores share the process' pool.
    explicit isocon_store(bool private_scratch = false) : own_pool(private_scratch ? new ScratchPool() : nullptr), pool(own_pool ? *own_pool : g_scratch) {}
    std::unique_ptr<ScratchPool> own_pool;
    ScratchPool &pool;
    std::vector<int32_t> lens;   // host copy
    uint64_t device_bytes = 0;
    uint64_t *d_planes = nullptr;
    // The four symbols of the set, code 0 .. 3.  "ACGT" for every shipped data set; a set over another alphabet of at most four
    // symbols (lower case, RNA) is packed under its own map: distances and the NN graph only compare symbols for equality, exactly
    // what edlib does with whatever characters it is given (EAM:111, NNG:105).  The entry points that emit letters or score with the
    // reference's "ACGT" matrix (alignments, consensus) refuse such a store (ISOCON_E_ALPHABET).
    char alphabet[4] = {'A', 'C', 'G', 'T'};
    bool acgt = true;
    // More than four distinct symbols (ACGT + N, mixed case ...): the planes hold the "ACGT" map with code 0 at every other byte, the
    // bytes themselves stay on the device and exc[i] marks the sequences that hold such a byte ("exceptional").  A pair with an
    // exceptional sequence is aligned by k_ed_bytes (ed_bytes.hpp) on the bytes; the bit-vector kernels never see it.
    uint8_t *d_bytes = nullptr;
    uint64_t *d_boff = nullptr;
    uint64_t bytes_base = 0;
    std::vector<uint8_t> exc;
    std::vector<uint32_t> exc_count;          // such bytes per sequence
    uint32_t n_exc = 0;
    bool is_exc(uint32_t i) const { return n_exc != 0 && exc[i] != 0; }
    int32_t *d_lens = nullptr;
    int32_t maxlen = 0;
    uint64_t last_host_waits = 0;          // isocon_nn_last_host_waits
};

namespace {

// A device buffer: pooled (slot of the store's ScratchPool) when constructed with a pool, private otherwise.
// Pinned staging for host<->device copies.  hipMemcpy on pageable memory pins the user pages on the fly and releases
// them lazily: measured 17-27 ms showing up at the NEXT synchronisation after a 7 MB hit-list download.  One pinned
// buffer per process, copies go through it in pieces.
struct PinnedStage {
    void *p = nullptr;
    size_t cap = 0;
    void *get(size_t bytes)
    {
        if (cap < bytes) {
            if (p) (void)hipHostFree(p);
            p = nullptr; cap = 0;
            if (hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess) cap = bytes;
            else { p = nullptr; (void)hipGetLastError(); }
        }
        return p;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};
static PinnedStage g_stage;
static constexpr size_t kStageBytes = (size_t)32 << 20;
static constexpr uint64_t kPackWaves = (uint64_t)1 << 25;          // wavefronts per packing launch (one per 64 bases of a sequence): below 2^32 threads
static constexpr size_t kStageMin = (size_t)32 << 10;      // smaller copies: the runtime's own staging path is fine

// Host buffers handed out by isocon_host_alloc are pinned: copies to / from them need no staging.
static std::vector<std::pair<const char *, size_t>> g_pinned;
static bool is_pinned(const void *p, size_t bytes)
{
    for (const auto &r : g_pinned)
        if ((const char *)p >= r.first && (const char *)p + bytes <= r.first + r.second) return true;
    return false;
}

// Blocking host waits of the entry point that is running -- every synchronous copy or memset, every event or device synchronise that
// the nearest-neighbour paths issue goes through one of the helpers below (isocon_nn_last_host_waits reports the last call's count).
static thread_local uint64_t g_host_waits = 0;
static hipError_t memcpy_wait(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) { ++g_host_waits; return hipMemcpy(dst, src, bytes, kind); }
static hipError_t memset_wait(void *dst, int value, size_t bytes) { ++g_host_waits; return hipMemset(dst, value, bytes); }
static hipError_t device_wait() { ++g_host_waits; return hipDeviceSynchronize(); }

static hipError_t copy_d2h(void *dst, const void *dsrc, size_t bytes)
{
    if (bytes < kStageMin || is_pinned(dst, bytes)) return memcpy_wait(dst, dsrc, bytes, hipMemcpyDeviceToHost);
    char *st = static_cast<char *>(g_stage.get(kStageBytes));
    if (!st) return memcpy_wait(dst, dsrc, bytes, hipMemcpyDeviceToHost);
    for (size_t off = 0; off < bytes; off += kStageBytes) {
        const size_t len = std::min(kStageBytes, bytes - off);
        const hipError_t e = memcpy_wait(st, static_cast<const char *>(dsrc) + off, len, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        memcpy(static_cast<char *>(dst) + off, st, len);
    }
    return hipSuccess;
}

static hipError_t copy_h2d(void *ddst, const void *src, size_t bytes)
{
    if (bytes < kStageMin || is_pinned(src, bytes)) return memcpy_wait(ddst, src, bytes, hipMemcpyHostToDevice);
    char *st = static_cast<char *>(g_stage.get(kStageBytes));
    if (!st) return memcpy_wait(ddst, src, bytes, hipMemcpyHostToDevice);
    for (size_t off = 0; off < bytes; off += kStageBytes) {
        const size_t len = std::min(kStageBytes, bytes - off);
        memcpy(st, static_cast<const char *>(src) + off, len);
        const hipError_t e = memcpy_wait(static_cast<char *>(ddst) + off, st, len, hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The one side stream of the library: the row layout of the bound matrix (NNContext::build_bounds) goes up on it from pinned memory of
// its own while the profile kernel runs on the null stream, followed by the small launches and fills that only depend on it (the
// transposed matrix' row layout, the seed arrays); the null stream then waits for `done` once, in front of k_qgram_mm.
// Like g_stage it is the process' only one and takes no lock: one process drives one device and runs one search at a time.
struct SideUpload {
    hipStream_t stream = nullptr;
    hipEvent_t before = nullptr, done = nullptr;
    PinnedStage pinned;
    bool in_flight = false;
    bool ready()
    {
        if (stream) return true;
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) { stream = nullptr; (void)hipGetLastError(); return false; }
        if (hipEventCreateWithFlags(&before, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            release();
            return false;
        }
        return true;
    }
    // the pinned block may be written again once the copies that read it are through
    void settle()
    {
        if (!in_flight) return;
        // (a call that failed between its first copy and the record of `done` leaves an event that says nothing: the stream itself is asked)
        if (hipEventQuery(done) != hipSuccess || hipStreamQuery(stream) != hipSuccess) { (void)hipGetLastError(); ++g_host_waits; (void)hipStreamSynchronize(stream); }
        in_flight = false;
    }
    void release()
    {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        if (before) (void)hipEventDestroy(before);
        if (done) (void)hipEventDestroy(done);
        stream = nullptr; before = done = nullptr; in_flight = false;
        pinned.release();
    }
};
static SideUpload g_side;

struct DevBuf {
    void *p = nullptr;
    ScratchPool *pool = nullptr;
    int slot = -1;
    DevBuf() {}
    DevBuf(ScratchPool *pl, int sl) : pool(pl), slot(sl) {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p && !pool) (void)hipFree(p); }
    template <class T> T *as() { return static_cast<T *>(p); }
    int alloc(size_t bytes)
    {
        if (pool) {
            p = pool->get(slot, bytes);
            if (!p) { g_last_error = "hipMalloc(scratch slot " + std::to_string(slot) + ", " + std::to_string(bytes) + " B) failed"; return ISOCON_E_HIP; }
            return ISOCON_OK;
        }
        if (p) { (void)hipFree(p); p = nullptr; }
        ISO_HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16));
        return ISOCON_OK;
    }
    // alloc + the host array's copy up
    int upload(const void *src, size_t bytes)
    {
        if (int rc = alloc(bytes)) return rc;
        ISO_HIP_CHECK(copy_h2d(p, src, bytes));
        return ISOCON_OK;
    }
};

// out[0 .. n] = exclusive prefix sums of f(in[i]) (common.hpp: k_scan_tiles + k_scan_finish), on `stream`.  A scan on another stream than
// the null stream has scratch slots of its own: one on the null stream may be in flight at the same time.
template <int SHIFT, class OUT>
static int device_exscan(ScratchPool *pl, const uint32_t *d_in, uint32_t n, OUT *d_out, hipStream_t stream = 0)
{
    DevBuf d_tmp(pl, stream ? SLOT_SCAN_TMP_SIDE : SLOT_SCAN_TMP), d_sums(pl, stream ? SLOT_SCAN_SUMS_SIDE : SLOT_SCAN_SUMS);
    const uint32_t tiles = std::max<uint32_t>(1, (n + SCAN_TILE - 1) / SCAN_TILE);
    int rc;
    if ((rc = d_tmp.alloc((size_t)std::max<uint32_t>(n, 1) * 4)) || (rc = d_sums.alloc((size_t)tiles * 8))) return rc;
    hipLaunchKernelGGL((k_scan_tiles<SHIFT>), dim3(tiles), dim3(256), 0, stream, d_in, n, d_tmp.as<uint32_t>(), d_sums.as<unsigned long long>());
    hipLaunchKernelGGL((k_scan_finish<OUT>), dim3(tiles), dim3(256), 0, stream, d_tmp.as<uint32_t>(), n, d_sums.as<unsigned long long>(), tiles, d_out, (unsigned long long *)nullptr);
    ISO_HIP_CHECK(hipGetLastError());
    return ISOCON_OK;
}

// Events of the phase timers: created once, handed out and taken back (a call records ~30 of them; hipEventCreate per interval would
// cost more than the waits the deferred timing removes).
struct EventPool {
    std::mutex mu;
    std::vector<hipEvent_t> idle;
    hipEvent_t get()
    {
        {
            std::lock_guard<std::mutex> g(mu);
            if (!idle.empty()) { hipEvent_t e = idle.back(); idle.pop_back(); return e; }
        }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return e;
    }
    void put(hipEvent_t e)
    {
        if (!e) return;
        std::lock_guard<std::mutex> g(mu);
        idle.push_back(e);
    }
    void release()
    {
        std::lock_guard<std::mutex> g(mu);
        for (hipEvent_t e : idle) (void)hipEventDestroy(e);
        idle.clear();
    }
};
static EventPool g_events;

// HIP-event time of the launches between start() and a stop.  start(), mark() and stop_later() only record events on the null stream:
// every interval owns its events, and resolve() -- once per entry point, behind a wait the call needs anyway -- turns the intervals
// into milliseconds: each is added to `total`, to the field its stop_later() named, and the part behind its mark() to the second
// field (to `marked_total` when none was named).  stop() is the blocking form: it resolves at once and returns its interval.
// ISOCON_DEBUG_VARIANT=nn_sync_phases: every stop_later() waits, as every phase did before the intervals were deferred (A/B runs, tests).
struct EventTimer {
    struct Interval { hipEvent_t e0, em, e1; float *acc, *marked_acc; };
    std::vector<Interval> pending;
    hipEvent_t e0 = nullptr, em = nullptr;          // of the open interval
    float total = 0.f;
    float marked_total = 0.f;
    const bool sync_phases = variant("nn_sync_phases");
    EventTimer() {}
    EventTimer(const EventTimer &) = delete;
    EventTimer &operator=(const EventTimer &) = delete;
    ~EventTimer()
    {
        g_events.put(e0); g_events.put(em);
        for (const Interval &iv : pending) { g_events.put(iv.e0); g_events.put(iv.em); g_events.put(iv.e1); }
    }
    void start()
    {
        g_events.put(em); em = nullptr;
        if (!e0) e0 = g_events.get();
        if (e0) (void)hipEventRecord(e0, 0);
    }
    void mark()
    {
        if (!e0) return;
        if (!em) em = g_events.get();
        if (em) (void)hipEventRecord(em, 0);
    }
    void stop_later(float *acc, float *marked_acc = nullptr)
    {
        if (!e0) return;
        hipEvent_t e1 = g_events.get();
        if (!e1) { g_events.put(e0); g_events.put(em); e0 = em = nullptr; return; }
        (void)hipEventRecord(e1, 0);
        pending.push_back(Interval{e0, em, e1, acc, marked_acc});
        e0 = em = nullptr;
        if (sync_phases) resolve(true);
    }
    // the pointers handed to stop_later() must still be good here
    void resolve(bool wait_counts = false)
    {
        if (pending.empty()) return;
        hipEvent_t last = pending.back().e1;          // (one stream: the last recorded event completes last)
        if (wait_counts || hipEventQuery(last) != hipSuccess) { (void)hipGetLastError(); ++g_host_waits; (void)hipEventSynchronize(last); }
        for (const Interval &iv : pending) {
            float ms = 0.f, part = 0.f;
            if (hipEventElapsedTime(&ms, iv.e0, iv.e1) != hipSuccess) { (void)hipGetLastError(); ms = 0.f; }
            total += ms;
            if (iv.acc) *iv.acc += ms;
            if (iv.em) {
                if (hipEventElapsedTime(&part, iv.em, iv.e1) != hipSuccess) { (void)hipGetLastError(); part = 0.f; }
                if (iv.marked_acc) *iv.marked_acc += part; else marked_total += part;
            }
            g_events.put(iv.e0); g_events.put(iv.em); g_events.put(iv.e1);
        }
        pending.clear();
    }
    float stop()
    {
        float ms = 0.f;
        stop_later(&ms);
        resolve(true);
        return ms;
    }
};

// Packs ASCII sequences into the store's bit-planes: one wavefront per (sequence, 64-base chunk) -- a coalesced 64-byte load,
// the two code bits of every base become the chunk's two words through two ballots.  *first_bad receives the smallest
// (sequence << 32 | position) holding a symbol outside ACGT.
struct PackMap { uint8_t sym[4]; };

// how often every byte value occurs in the uploaded sequences (only looked at when a symbol outside ACGT turned up)
__global__ __launch_bounds__(256) void k_byte_histogram(const uint8_t *__restrict__ ascii, uint64_t total, unsigned long long *__restrict__ hist)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) atomicAdd(&h[ascii[i]], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(hist + threadIdx.x, (unsigned long long)h[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_pack_planes(const uint8_t *__restrict__ ascii, const uint64_t *__restrict__ offsets, uint64_t base, uint32_t n,
                                                      uint32_t nchunks, uint64_t *__restrict__ planes, unsigned long long *__restrict__ first_bad, PackMap map,
                                                      uint32_t fold, uint64_t w0)
{
    const uint64_t w = w0 + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);          // (a launch holds fewer than 2^32 threads: w0 = first wavefront of this one)
    if (w >= (uint64_t)nchunks * n) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t chunk = (uint32_t)(w / n), seq = (uint32_t)(w % n);           // consecutive waves: consecutive sequences
    const uint64_t off = offsets[seq] - base, len = offsets[seq + 1] - offsets[seq];
    const uint64_t pos = (uint64_t)chunk * 64 + lane;
    int cd = 0;
    bool bad = false;
    if (pos < len) {
        uint8_t ch = ascii[off + pos];
        if (fold && ch >= 'a' && ch <= 'z') ch = (uint8_t)(ch - 32);          // fold: lower case takes its upper-case letter's code, any other byte code 0, nothing is reported
        cd = ch == map.sym[0] ? 0 : ch == map.sym[1] ? 1 : ch == map.sym[2] ? 2 : ch == map.sym[3] ? 3 : -1;
        bad = cd < 0 && !fold;
    }
    const unsigned long long lo = __ballot(!bad && (cd & 1)), hi = __ballot(!bad && (cd & 2)), bm = __ballot(bad);
    if (lane == 0) {
        planes[((size_t)chunk * n + seq) * 2] = lo;
        planes[((size_t)chunk * n + seq) * 2 + 1] = hi;
        if (bm) atomicMin(first_bad, ((unsigned long long)seq << 32) | ((unsigned long long)chunk * 64 + (unsigned long long)(__ffsll((long long)bm) - 1)));
    }
}

// The steps of a store's creation (store_create_impl below).  PackJob: what the packing launches of one creation read.  Scratch (ASCII, offsets, first bad position) comes from the process-wide pool.
struct PackJob {
    DevBuf d_ascii{&g_scratch, SLOT_PACK_ASCII}, d_off{&g_scratch, SLOT_PACK_OFF}, d_bad{&g_scratch, SLOT_PACK_BAD};
    uint64_t base = 0, total = 0;          // first byte of the set in the caller's offsets, bytes of the set
    uint32_t n = 0, nchunks = 0;
    uint64_t pack_waves = kPackWaves;
};
constexpr unsigned long long kNoBad = ~0ull;

// every way out of a failed creation: the message, and the HIP error does not stay behind for the next call's check
int create_failed(const char *message)
{
    g_last_error = message;
    (void)hipGetLastError();
    return ISOCON_E_HIP;
}

// issue(grid, w0) for the job's nchunks * n wavefronts (four to a block), pack_waves of them a launch
template <class Issue>
void for_wave_slices(const PackJob &job, Issue issue)
{
    const uint64_t waves = (uint64_t)job.nchunks * job.n;
    for (uint64_t w0 = 0; w0 < waves; w0 += job.pack_waves) issue(dim3((unsigned)((std::min<uint64_t>(job.pack_waves, waves - w0) + 3) / 4)), w0);
}

// packs under `map`; fold == 0: *bad = the first position that holds a symbol outside it (kNoBad: none); fold == 1 reports nothing, bad == nullptr
bool pack_planes(PackJob &job, uint64_t *planes, PackMap map, uint32_t fold, unsigned long long *bad)
{
    if (bad && hipMemcpy(job.d_bad.p, &kNoBad, 8, hipMemcpyHostToDevice) != hipSuccess) return false;
    for_wave_slices(job, [&](dim3 grid, uint64_t w0) {
        hipLaunchKernelGGL(k_pack_planes, grid, dim3(256), 0, 0, job.d_ascii.as<uint8_t>(), job.d_off.as<uint64_t>(), job.base, job.n, job.nchunks, planes,
                           job.d_bad.as<unsigned long long>(), map, fold, w0);
    });
    return hipGetLastError() == hipSuccess && (!bad || hipMemcpy(bad, job.d_bad.p, 8, hipMemcpyDeviceToHost) == hipSuccess);
}

// The sequences at seq_ptrs[i] (offsets: the prefix sums of their lengths) -> d_dst as their concatenation, gathered into the two halves of the
// pinned staging buffer: one half on its way to the device while the other is being filled.
bool upload_gathered(char *d_dst, const uint8_t *const *seq_ptrs, const uint64_t *offsets, uint32_t n, uint64_t total)
{
    char *stg = static_cast<char *>(g_stage.get(kStageBytes));
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool up = stg != nullptr && hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) == hipSuccess;
    const size_t half = kStageBytes / 2;
    uint64_t done = 0;           // bytes of the concatenation already sent
    bool busy[2] = {false, false};
    const unsigned hc = std::thread::hardware_concurrency();
    const unsigned n_thr = total >= ((uint64_t)8 << 20) ? std::min(4u, hc ? hc : 1u) : 1u;      // one thread copies ~10 GB/s: 125 MB at C3
    for (int h = 0; up && done < total; h ^= 1) {
        if (busy[h]) up = hipEventSynchronize(ev[h]) == hipSuccess;
        const size_t fill = (size_t)std::min<uint64_t>(half, total - done);
        if (n_thr <= 1) gather_bytes(stg + h * half, seq_ptrs, offsets, n, done, done + fill);
        else {
            std::thread th[4];
            const size_t part = (fill + n_thr - 1) / n_thr;
            for (unsigned t = 0; t < n_thr; ++t) {
                const size_t a = std::min(fill, t * part), b = std::min(fill, (t + 1) * part);
                th[t] = std::thread([=] { if (b > a) gather_bytes(stg + h * half + a, seq_ptrs, offsets, n, done + a, done + b); });
            }
            for (unsigned t = 0; t < n_thr; ++t) th[t].join();
        }
        up = up && hipMemcpyAsync(d_dst + done, stg + h * half, fill, hipMemcpyHostToDevice, 0) == hipSuccess && hipEventRecord(ev[h], 0) == hipSuccess;
        busy[h] = true;
        done += fill;
    }
    up = up && hipStreamSynchronize(0) == hipSuccess;
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    return up;
}

// how often every byte value occurs in the set
bool byte_histogram(PackJob &job, unsigned long long (&hist)[256])
{
    DevBuf d_hist(&g_scratch, SLOT_PACK_HIST);
    if (d_hist.alloc(256 * 8) != ISOCON_OK || hipMemset(d_hist.p, 0, 256 * 8) != hipSuccess) return false;
    hipLaunchKernelGGL(k_byte_histogram, dim3(1024), dim3(256), 0, 0, job.d_ascii.as<uint8_t>(), job.total, d_hist.as<unsigned long long>());
    return hipGetLastError() == hipSuccess && hipMemcpy(hist, d_hist.p, sizeof(hist), hipMemcpyDeviceToHost) == hipSuccess;
}

// More than four symbols: keep the bytes.
// Planes: the "ACGT" map with lower case folded onto upper case and code 0 at every other byte.  For the pairs of ordinary
// sequences they are what they always are; for a sequence with other bytes they hold its image under a map that MERGES symbol
// classes, and merging classes can only turn mismatches into matches: d(image x, image y) <= d(x, y), so every lower bound
// computed on the planes (q-gram bounds) holds for the sequences themselves.
// The bytes and their offsets move from the scratch pool into the store, with one count per sequence.
bool keep_bytes(isocon_store &st, PackJob &job)
{
    const uint32_t n = job.n, nn = std::max<uint32_t>(n, 1);
    DevBuf d_flags(&g_scratch, SLOT_PACK_FLAGS);
    st.exc.assign(nn, 0);
    st.exc_count.assign(nn, 0);
    if (d_flags.alloc((size_t)nn * 4) != ISOCON_OK || hipMemset(d_flags.p, 0, (size_t)nn * 4) != hipSuccess ||
        hipMalloc((void **)&st.d_bytes, job.total ? job.total : 16) != hipSuccess || hipMalloc((void **)&st.d_boff, (size_t)(nn + 1) * 8) != hipSuccess)
        return false;
    if (!pack_planes(job, st.d_planes, PackMap{{'A', 'C', 'G', 'T'}}, 1u, nullptr)) return false;
    for_wave_slices(job, [&](dim3 grid, uint64_t w0) {
        hipLaunchKernelGGL(k_exception_flags, grid, dim3(256), 0, 0, job.d_ascii.as<uint8_t>(), job.d_off.as<uint64_t>(), job.base, n, job.nchunks, d_flags.as<uint32_t>(),
                           (uint32_t)'A' | ((uint32_t)'C' << 8) | ((uint32_t)'G' << 16) | ((uint32_t)'T' << 24), w0);
    });
    if (hipGetLastError() != hipSuccess || hipMemcpy(st.exc_count.data(), d_flags.p, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(st.d_bytes, job.d_ascii.p, job.total, hipMemcpyDeviceToDevice) != hipSuccess ||
        hipMemcpy(st.d_boff, job.d_off.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToDevice) != hipSuccess)
        return false;
    st.bytes_base = job.base;
    for (uint32_t i = 0; i < n; ++i) { st.exc[i] = st.exc_count[i] != 0; st.n_exc += st.exc[i]; }
    st.acgt = false;
    st.device_bytes += job.total + (size_t)(nn + 1) * 8;
    return true;
}

// At most four symbols, not all of them ACGT: the set is packed again under its own map -- A, C, G, T keep their codes if present, the other
// symbols take the free codes in byte order -- and serves the distance / NN entry points.
bool pack_own_alphabet(isocon_store &st, PackJob &job, const unsigned long long (&hist)[256])
{
    PackMap map{{0, 0, 0, 0}};
    bool used[4] = {false, false, false, false};
    const char acgt_sym[4] = {'A', 'C', 'G', 'T'};
    for (int k = 0; k < 4; ++k) if (hist[(uint8_t)acgt_sym[k]]) { map.sym[k] = (uint8_t)acgt_sym[k]; used[k] = true; }
    for (int c = 0; c < 256; ++c) {
        if (!hist[c] || c == 'A' || c == 'C' || c == 'G' || c == 'T') continue;
        for (int k = 0; k < 4; ++k) if (!used[k]) { map.sym[k] = (uint8_t)c; used[k] = true; break; }
    }
    // (free codes keep byte 0, which no sequence holds: C strings)  -- a 0 byte in the input would be one of the four symbols
    for (int k = 0; k < 4; ++k) if (!used[k]) { for (int c = 1; c < 256; ++c) if (!hist[c] && c != map.sym[0] && c != map.sym[1] && c != map.sym[2] && c != map.sym[3]) { map.sym[k] = (uint8_t)c; break; } }
    unsigned long long bad;
    if (!pack_planes(job, st.d_planes, map, 0u, &bad) || bad != kNoBad) return false;
    for (int k = 0; k < 4; ++k) st.alphabet[k] = (char)map.sym[k];
    st.acgt = false;
    return true;
}

}  // namespace

extern "C" {

const char *isocon_strerror(int status)
{
    switch (status) {
    case ISOCON_OK: return "ok";
    case ISOCON_E_ARG: return "bad argument";
    case ISOCON_E_ALPHABET: return "sequence contains a symbol outside ACGT";
    case ISOCON_E_HIP: return "HIP runtime error";
    case ISOCON_E_CAPACITY: return "output buffer too small";
    case ISOCON_E_NODEVICE: return "no usable GPU";
    case ISOCON_E_UNSUPPORTED: return "unsupported request";
    default: return "unknown status";
    }
}

const char *isocon_last_error(void) { return g_last_error.c_str(); }

int isocon_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void isocon_release_scratch(void) { g_scratch.release(); g_stage.release(); g_events.release(); g_side.release(); }

int isocon_init(int device_ordinal)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { g_last_error = "hipGetDeviceCount: no device"; return ISOCON_E_NODEVICE; }
    if (device_ordinal < 0 || device_ordinal >= n) return ISOCON_E_ARG;
    ISO_HIP_CHECK(hipSetDevice(device_ordinal));
    return ISOCON_OK;
}

// ascii != nullptr: one contiguous buffer addressed by offsets; else the sequences lie at seq_ptrs[i] (offsets still hold the prefix
// sums of their lengths) and are gathered into the two halves of the pinned staging buffer, one half on its way to the device
// while the other is being filled.
static int store_create_impl(const uint8_t *ascii, const uint8_t *const *seq_ptrs, const uint64_t *offsets, uint32_t n, isocon_store **out, bool private_scratch = false)
{
    *out = nullptr;
    int32_t maxlen = 0;
    const uint32_t nn = std::max<uint32_t>(n, 1);
    std::vector<int32_t> lens(nn, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0x3fffffff) return ISOCON_E_ARG;
        lens[i] = (int32_t)(offsets[i + 1] - offsets[i]);
        maxlen = std::max(maxlen, lens[i]);
    }
    const uint32_t nchunks = (uint32_t)((maxlen + 63) / 64 + 1);
    const uint64_t base = n ? offsets[0] : 0, total = n ? offsets[n] - offsets[0] : 0;
    // the store is destroyed on every way out but the last line
    std::unique_ptr<isocon_store, decltype(&isocon_store_destroy)> st(new isocon_store(private_scratch), isocon_store_destroy);
    st->lens = lens;
    st->maxlen = maxlen;
    const size_t pbytes = (size_t)nchunks * nn * 2 * sizeof(uint64_t), lbytes = lens.size() * sizeof(int32_t);
    if (hipMalloc((void **)&st->d_planes, pbytes) != hipSuccess || hipMalloc((void **)&st->d_lens, lbytes) != hipSuccess) return create_failed("hipMalloc(store) failed");
    // The bytes go to the device as they are and are packed there (k_pack_planes: one wavefront per 64 bases, two ballots);
    // the host only checked the offsets.
    PackJob job;
    job.base = base; job.total = total; job.n = n; job.nchunks = nchunks;
    if (const char *e = variant_value("pack_waves")) job.pack_waves = std::max<uint64_t>(4, strtoull(e, nullptr, 10)) & ~(uint64_t)3;      // tests: many launches on a small set
    int rc;
    if ((rc = job.d_ascii.alloc(total ? total : 16)) || (rc = job.d_off.alloc((size_t)(nn + 1) * 8)) || (rc = job.d_bad.alloc(8))) return rc;
    bool ok = !total || (ascii ? copy_h2d(job.d_ascii.p, ascii + base, total) == hipSuccess : upload_gathered(job.d_ascii.as<char>(), seq_ptrs, offsets, n, total));
    ok = ok && (n == 0 || copy_h2d(job.d_off.p, offsets, (size_t)(n + 1) * 8) == hipSuccess) && copy_h2d(st->d_lens, lens.data(), lbytes) == hipSuccess;
    unsigned long long bad = kNoBad;
    if (ok) ok = n ? pack_planes(job, st->d_planes, PackMap{{'A', 'C', 'G', 'T'}}, 0u, &bad) : hipMemset(st->d_planes, 0, pbytes) == hipSuccess;
    if (!ok) return create_failed("isocon_store_create: device copy / packing failed");
    if (bad != kNoBad) {
        // A symbol outside ACGT.  edlib takes any characters (EAM:111, NNG:105): if the whole set uses at most four distinct symbols
        // (lower case, RNA ...) it is packed again under its own map; more than four symbols cannot be held in 2 bits.
        unsigned long long hist[256];
        if (!byte_histogram(job, hist)) return create_failed("isocon_store_create: symbol histogram failed");
        int distinct = 0;
        for (int c = 0; c < 256; ++c) distinct += hist[c] != 0;
        if (distinct > 4) {
            if (!keep_bytes(*st, job)) return create_failed("isocon_store_create: keeping the bytes of a set with more than four symbols failed");
        } else if (!pack_own_alphabet(*st, job, hist)) return create_failed("isocon_store_create: packing under the set's own alphabet failed");
    }
    st->device_bytes += pbytes + lbytes;
    st->dev.planes = st->d_planes;
    st->dev.il = nullptr;
    st->dev.lens = st->d_lens;
    st->dev.n = n;
    st->dev.nchunks = nchunks;
    st->lens.resize(n);
    *out = st.release();
    return ISOCON_OK;
}

int isocon_store_create(const uint8_t *ascii, const uint64_t *offsets, uint32_t n, isocon_store **out)
{
    if (!out || (!ascii && n) || !offsets) return ISOCON_E_ARG;
    return store_create_impl(ascii, nullptr, offsets, n, out);
}

int isocon_store_create_ptrs(const uint8_t *const *seq_ptrs, const uint64_t *seq_lens, uint32_t n, isocon_store **out)
{
    return isocon_store_create_ptrs_ex(seq_ptrs, seq_lens, n, 0u, out);
}

int isocon_store_create_ptrs_ex(const uint8_t *const *seq_ptrs, const uint64_t *seq_lens, uint32_t n, uint32_t flags, isocon_store **out)
{
    if (!out || (n && (!seq_ptrs || !seq_lens)) || (flags & ~(uint32_t)ISOCON_STORE_PRIVATE_SCRATCH)) return ISOCON_E_ARG;
    std::vector<uint64_t> offsets((size_t)n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (seq_lens[i] && !seq_ptrs[i]) return ISOCON_E_ARG;
        offsets[i + 1] = offsets[i] + seq_lens[i];
    }
    return store_create_impl(nullptr, seq_ptrs, offsets.data(), n, out, (flags & ISOCON_STORE_PRIVATE_SCRATCH) != 0);
}

void *isocon_host_alloc(uint64_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    g_pinned.emplace_back((const char *)p, (size_t)(bytes ? bytes : 16));
    return p;
}

void isocon_host_free(void *p)
{
    if (!p) return;
    for (size_t i = 0; i < g_pinned.size(); ++i)
        if (g_pinned[i].first == (const char *)p) { g_pinned.erase(g_pinned.begin() + (long)i); break; }
    (void)hipHostFree(p);
}

void isocon_store_destroy(isocon_store *s)
{
    if (!s) return;
    if (s->d_planes) (void)hipFree(s->d_planes);
    if (s->d_lens) (void)hipFree(s->d_lens);
    if (s->d_bytes) (void)hipFree(s->d_bytes);
    if (s->d_boff) (void)hipFree(s->d_boff);
    if (s->own_pool) s->own_pool->release();
    delete s;
}

uint32_t isocon_store_size(const isocon_store *s) { return s ? s->dev.n : 0; }
uint64_t isocon_nn_last_host_waits(const isocon_store *s) { return s ? s->last_host_waits : 0; }
uint64_t isocon_store_device_bytes(const isocon_store *s) { return s ? s->device_bytes : 0; }

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// explicit pair lists
// ---------------------------------------------------------------------------------------------------------------
namespace {

// The stages of a pair list on the device: the three of ed_pairs_plan.hpp and the byte-wise one in front of them.
struct DeviceStages {
    using Ids = std::vector<uint32_t>;
    using Ints = std::vector<int32_t>;
    isocon_store *st;
    EventTimer &tm;
    // One stage: its three input arrays go up into the scratch slots slot0 .. slot0 + 2, `launch(in0, in1, in2, out)` issues the kernel between
    // the timer's events (kernel_ms: the launches, copies excluded), n_out answers come down through slot0 + 3.
    template <class Launch>
    int run(int slot0, const Ids &in0, const Ids &in1, const Ints &in2, size_t n_out, Ints &out, Launch launch)
    {
        static_assert(SLOT_ED_OUT == SLOT_ED_TS + 3 && SLOT_FULL_OUT == SLOT_FULL_A + 3 && SLOT_EB_OUT == SLOT_EB_A + 3, "a stage's four slots are consecutive");
        out.assign(n_out, -1);
        if (!n_out) return ISOCON_OK;
        DevBuf d0(&st->pool, slot0), d1(&st->pool, slot0 + 1), d2(&st->pool, slot0 + 2), d_out(&st->pool, slot0 + 3);
        int rc;
        if ((rc = d0.upload(in0.data(), in0.size() * 4)) || (rc = d1.upload(in1.data(), in1.size() * 4)) || (rc = d2.upload(in2.data(), in2.size() * 4)) || (rc = d_out.alloc(n_out * 4)))
            return rc;
        tm.start();
        launch(d0.as<uint32_t>(), d1.as<uint32_t>(), d2.as<int32_t>(), d_out.as<int32_t>());
        ISO_HIP_CHECK(hipGetLastError());
        tm.stop();
        ISO_HIP_CHECK(copy_d2h(out.data(), d_out.p, n_out * 4));
        return ISOCON_OK;
    }
    // (shares the tiles' slots: the two never hold data at the same time)
    int lanes(const Ids &a, const Ids &b, const Ints &k, Ints &out)
    {
        const size_t np = a.size();
        NNParams none;
        memset(&none, 0, sizeof(none));
        return run(SLOT_ED_TS, a, b, k, np, out, [&](uint32_t *da, uint32_t *db, int32_t *dk, int32_t *res) {
            hipLaunchKernelGGL(k_ed_lanes<false>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, 0, st->dev, none, da, db, dk, (uint64_t)np, res);
        });
    }
    int tiles(int W, const Ids &tile_shared, const Ids &lane_ids, const Ints &lane_k, Ints &out)
    {
        const auto kernel = W == 1 ? k_ed_band_tiles<1> : W == 2 ? k_ed_band_tiles<2> : W == 4 ? k_ed_band_tiles<4> : W == 8 ? k_ed_band_tiles<8> : nullptr;
        if (!kernel) return ISOCON_E_ARG;
        const size_t nt = tile_shared.size();
        return run(SLOT_ED_TS, tile_shared, lane_ids, lane_k, nt * 64, out, [&](uint32_t *ts, uint32_t *ids, int32_t *ks, int32_t *res) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, 0, st->dev, ts, ids, ks, res, (uint32_t)nt);
        });
    }
    int full(const Ids &a, const Ids &b, const Ints &k, Ints &out)
    {
        const size_t np = a.size();
        bool multipass = false;
        int32_t maxtext = 0;
        for (size_t p = 0; p < np; ++p) {
            const int32_t la = st->lens[a[p]], lb = st->lens[b[p]];
            if (std::min(la, lb) > 4096) multipass = true;
            maxtext = std::max(maxtext, std::max(la, lb));
        }
        const size_t lds = multipass ? (size_t)((maxtext + 15) & ~15) : 0;
        if (lds > 160 * 1024) { g_last_error = "sequence longer than 163840 bases in the un-banded kernel"; return ISOCON_E_UNSUPPORTED; }
        if (lds > 64 * 1024)
            ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_ed_full, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        return run(SLOT_FULL_A, a, b, k, np, out, [&](uint32_t *da, uint32_t *db, int32_t *dk, int32_t *res) {
            hipLaunchKernelGGL(k_ed_full, dim3((unsigned)np), dim3(64), lds, 0, st->dev, da, db, dk, res, (uint32_t)np);
        });
    }
    // k < 0: unbounded.  One wavefront per pair, a grid of at most 8192 that strides over the list (each needs a row buffer).
    int bytes(const Ids &a, const Ids &b, const Ints &k, Ints &out)
    {
        const size_t np = a.size();          // (not 0: the caller has such pairs)
        if (!st->d_bytes) { g_last_error = "internal: byte-wise distances on a store that kept no bytes"; return ISOCON_E_HIP; }
        if (st->maxlen >= (int32_t)EB_INF - 1) { g_last_error = "byte-wise distances: sequences of 8 388 606 bases and more are not supported"; return ISOCON_E_UNSUPPORTED; }
        const uint32_t row_stride = (uint32_t)st->maxlen + 130u;
        size_t waves = std::min<size_t>(np, 8192);
        while (waves > 256 && waves * row_stride * 4 > ((size_t)2 << 30)) waves /= 2;
        DevBuf d_rows(&st->pool, SLOT_EB_ROWS);
        if (int rc = d_rows.alloc(waves * row_stride * 4)) return rc;
        return run(SLOT_EB_A, a, b, k, np, out, [&](uint32_t *da, uint32_t *db, int32_t *dk, int32_t *res) {
            hipLaunchKernelGGL(k_ed_bytes, dim3((unsigned)waves), dim3(64), 0, 0, ByteStore{st->d_bytes, st->d_boff, st->bytes_base, st->d_lens}, da, db, dk,
                               (unsigned long long)np, d_rows.as<uint32_t>(), row_stride, res);
        });
    }
};

}  // namespace

namespace isocon {

// Shared by isocon_ed_pairs and the NN fallback: exact bounded/unbounded distances for an explicit pair list.
// Stages: 64-row band (k <= 63), 128, 256, 512 rows, then the un-banded kernel; which pair goes where: ed_pairs_plan.hpp.
// images: distances of the sequences' IMAGES in the planes (a set with more than four symbols: lower bounds of the true distances, see
// isocon_store) -- the pairs of exceptional sequences are not split off to the byte-wise kernel.
int ed_pairs_impl(isocon_store *st, const uint32_t *a, const uint32_t *b, const int32_t *k, uint64_t n_pairs,
                  int32_t *out_ed, float *kernel_ms, uint64_t *full_pairs, bool images)
{
    EventTimer tm;
    DeviceStages stages{st, tm};
    const uint32_t n = st->dev.n;
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (a[p] >= n || b[p] >= n) return ISOCON_E_ARG;
    std::vector<uint64_t> pending;
    pending.reserve(n_pairs);
    if (st->n_exc && !images) {
        // pairs with a sequence that holds symbols outside the planes' map: on the bytes (ed_bytes.hpp), whatever their threshold
        std::vector<uint64_t> xp;
        for (uint64_t p = 0; p < n_pairs; ++p) (st->exc[a[p]] || st->exc[b[p]] ? xp : pending).push_back(p);
        if (!xp.empty()) {
            std::vector<uint32_t> xa(xp.size()), xb(xp.size());
            std::vector<int32_t> xk(xp.size()), res;
            for (size_t i = 0; i < xp.size(); ++i) { xa[i] = a[xp[i]]; xb[i] = b[xp[i]]; xk[i] = k ? k[xp[i]] : -1; }
            if (int rc = stages.bytes(xa, xb, xk, res)) return rc;
            for (size_t i = 0; i < xp.size(); ++i) out_ed[xp[i]] = res[i];
        }
    } else {
        pending.resize(n_pairs);
        std::iota(pending.begin(), pending.end(), 0);
    }
    // ISOCON_DEBUG_VARIANT=ed_lanes=1 / =0: all / none of the pairs one per lane, whatever the size of their group
    const char *e = variant_value("ed_lanes");
    const size_t min_group = e ? (atoi(e) ? (size_t)-1 : 0) : 16;
    if (int rc = ed_pairs_plan(st->lens.data(), n, a, b, k, n_pairs, std::move(pending), min_group, stages, out_ed, full_pairs, g_last_error)) return rc;
    if (kernel_ms) *kernel_ms = tm.total;
    return ISOCON_OK;
}

}  // namespace isocon

// 64-bit digest of the packed set (every plane word and every length, each mixed with its position): two stores have the
// same digest iff -- up to hash collisions -- they hold the same sequences in the same order.  Sharded runs compare it.
__global__ __launch_bounds__(256) void k_store_digest(const uint64_t *__restrict__ planes, size_t n_words, const int32_t *__restrict__ lens, uint32_t n,
                                                      unsigned long long *__restrict__ out)
{
    unsigned long long acc = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words + n; i += stride) {
        unsigned long long v = i < n_words ? planes[i] : (unsigned long long)(uint32_t)lens[i - n_words];
        v ^= (unsigned long long)i * 0xD6E8FEB86659FD93ull;
        v ^= v >> 32; v *= 0x9E3779B97F4A7C15ull; v ^= v >> 29; v *= 0xBF58476D1CE4E5B9ull; v ^= v >> 32;
        acc += v;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}

extern "C" int isocon_store_digest(const isocon_store *s, uint64_t *out)
{
    if (!s || !out) return ISOCON_E_ARG;
    DevBuf d_acc;
    int rc;
    if ((rc = d_acc.alloc(8))) return rc;
    ISO_HIP_CHECK(hipMemset(d_acc.p, 0, 8));
    const size_t n_words = (size_t)s->dev.nchunks * std::max<uint32_t>(s->dev.n, 1) * 2;
    hipLaunchKernelGGL(k_store_digest, dim3(1024), dim3(256), 0, 0, s->d_planes, n_words, s->d_lens, s->dev.n, d_acc.as<unsigned long long>());
    ISO_HIP_CHECK(hipGetLastError());
    ISO_HIP_CHECK(hipMemcpy(out, d_acc.p, 8, hipMemcpyDeviceToHost));
    return ISOCON_OK;
}

extern "C" int isocon_ed_pairs(isocon_store *s, const uint32_t *a, const uint32_t *b, const int32_t *k, uint64_t n_pairs,
                               int32_t *out_ed, float *kernel_ms)
{
    if (!s || (n_pairs && (!a || !b || !out_ed))) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    if (!n_pairs) return ISOCON_OK;
    return ed_pairs_impl(s, a, b, k, n_pairs, out_ed, kernel_ms, nullptr, false);
}

extern "C" int isocon_qgram_params(int32_t *out)
{
    if (out) { out[0] = QG_Q; out[1] = QG_B0; out[2] = QG_B1; out[3] = QG_CAP; }
    return QM_K;
}

// q-gram lower bounds of explicit pairs (qgram_mm.hpp), computed on the 2-bit planes
namespace isocon {
int qgram_bounds_for_pairs(isocon_store *s, const uint32_t *a, const uint32_t *b, uint64_t n_pairs, int32_t *out_bound, float *kernel_ms)
{
    const uint32_t n = s->dev.n;
    const uint32_t n_pad = std::max<uint32_t>(QM_TILE, ((n + QM_TILE - 1) / QM_TILE) * QM_TILE);
    DevBuf d_prof(&s->pool, SLOT_NN_QPROF), d_sum(&s->pool, SLOT_NN_QSUM), d_a(&s->pool, SLOT_ED_TS), d_b(&s->pool, SLOT_ED_IDS), d_out(&s->pool, SLOT_ED_OUT);
    int rc;
    if ((rc = d_prof.alloc((size_t)n_pad * (QM_K / 2))) || (rc = d_sum.alloc((size_t)n * 4)) || (rc = d_a.upload(a, n_pairs * 4)) ||
        (rc = d_b.upload(b, n_pairs * 4)) || (rc = d_out.alloc(n_pairs * 4)))
        return rc;
    s->pool.bound_tag.valid = false;          // the profile slot is shared with the bound matrix builds
    EventTimer tm;
    tm.start();
    hipLaunchKernelGGL(k_qgram_profile4, dim3((n + QP_SEQS - 1) / QP_SEQS), dim3(256), 0, 0, s->dev, d_prof.as<uint8_t>(), d_sum.as<uint32_t>(), n_pad,
                       (uint32_t *)nullptr, 0u);
    ISO_HIP_CHECK(hipGetLastError());
    // (a launch holds fewer than 2^32 threads: 2^24 pairs per launch)
    for (uint64_t at = 0; at < n_pairs; at += (uint64_t)1 << 24) {
        const uint64_t cnt = std::min<uint64_t>((uint64_t)1 << 24, n_pairs - at);
        hipLaunchKernelGGL(k_qgram_lb_pairs, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, 0, d_prof.as<uint8_t>(), d_sum.as<uint32_t>(), n_pad, d_a.as<uint32_t>() + at,
                           d_b.as<uint32_t>() + at, cnt, d_out.as<int32_t>() + at);
        ISO_HIP_CHECK(hipGetLastError());
    }
    const float ms = tm.stop();
    if (kernel_ms) *kernel_ms = ms;
    ISO_HIP_CHECK(copy_d2h(out_bound, d_out.p, n_pairs * 4));
    return ISOCON_OK;
}
}  // namespace isocon

// ... exposed for tests: what the main pass of the NN search consults
extern "C" int isocon_qgram_bound_pairs(isocon_store *s, const uint32_t *a, const uint32_t *b, uint64_t n_pairs, int32_t *out_bound)
{
    if (!s || (n_pairs && (!a || !b || !out_bound))) return ISOCON_E_ARG;
    if (!n_pairs) return ISOCON_OK;
    if (s->n_exc) { g_last_error = "q-gram bounds are defined on the 2-bit planes: the set holds more than four distinct symbols"; return ISOCON_E_ALPHABET; }
    const uint32_t n = s->dev.n;
    for (uint64_t i = 0; i < n_pairs; ++i)
        if (a[i] >= n || b[i] >= n) { g_last_error = "pair index out of range"; return ISOCON_E_ARG; }
    return qgram_bounds_for_pairs(s, a, b, n_pairs, out_bound, nullptr);
}

// ... and the block bound behind it (nn_filter.hpp), one workgroup per pair
extern "C" int isocon_block_bound_pairs(isocon_store *s, const uint32_t *owner, const uint32_t *partner, uint64_t n_pairs, int32_t probe_stride, int32_t *out_count)
{
    if (probe_stride != 4 && probe_stride != 2) return ISOCON_E_ARG;
    if (!s || (n_pairs && (!owner || !partner || !out_count))) return ISOCON_E_ARG;
    if (!n_pairs) return ISOCON_OK;
    if (s->n_exc) { g_last_error = "block bounds are defined on the 2-bit planes: the set holds more than four distinct symbols"; return ISOCON_E_ALPHABET; }
    const uint32_t n = s->dev.n;
    if (n_pairs >= ((uint64_t)1 << 31)) return ISOCON_E_ARG;
    for (uint64_t i = 0; i < n_pairs; ++i)
        if (owner[i] >= n || partner[i] >= n) { g_last_error = "pair index out of range"; return ISOCON_E_ARG; }
    const uint32_t stride = nnf_text2_stride(s->maxlen);
    DevBuf d_text(&s->pool, SLOT_NN_TEXT2), d_a(&s->pool, SLOT_ED_TS), d_b(&s->pool, SLOT_ED_IDS), d_out(&s->pool, SLOT_ED_OUT);
    int rc;
    if ((rc = d_text.alloc((size_t)n * stride * 4)) || (rc = d_a.upload(owner, n_pairs * 4)) || (rc = d_b.upload(partner, n_pairs * 4)) || (rc = d_out.alloc(n_pairs * 4)))
        return rc;
    hipLaunchKernelGGL(k_build_text2, dim3(n), dim3(256), 0, 0, s->dev, d_text.as<uint32_t>(), stride);
    hipLaunchKernelGGL(k_nn_block_count_pairs, dim3((unsigned)n_pairs), dim3(256), 0, 0, d_text.as<uint32_t>(), stride, s->dev.lens, d_a.as<uint32_t>(), d_b.as<uint32_t>(), d_out.as<int32_t>(), probe_stride);
    ISO_HIP_CHECK(hipGetLastError());
    ISO_HIP_CHECK(copy_d2h(out_count, d_out.p, n_pairs * 4));
    return ISOCON_OK;
}

// ... and the two kernels of the main pass that apply it, on chunks the caller made (tests): the buffers are laid out as NNContext::plan_lists
// lays them out and the launches are its own (nnf_launch_filter); every capacity holds the worst case, so the kernels never report an overflow
extern "C" int isocon_block_filter_chunks(isocon_store *s, const int32_t *thr, uint32_t n_chunks, const uint32_t *owner, const uint8_t *narrow, const uint64_t *chunk_ptr,
                                          const uint32_t *words, int32_t kcap, uint32_t list_min, int32_t second_pass, uint32_t *out_slot, uint32_t *out_count,
                                          uint64_t *out_begin, uint64_t chunks_cap, uint32_t *out_list, uint64_t list_cap, uint32_t *out_pa, uint32_t *out_pb, uint64_t pairs_cap,
                                          uint64_t *out_counters)
{
    if (!s || !out_counters || (second_pass != 0 && second_pass != 1) || list_min == 0) return ISOCON_E_ARG;
    for (int i = 0; i < 9; ++i) out_counters[i] = 0;
    if (!n_chunks) return ISOCON_OK;
    if (!thr || !owner || !narrow || !chunk_ptr || !words || !out_slot || !out_count || !out_begin || !out_list || !out_pa || !out_pb) return ISOCON_E_ARG;
    if (s->n_exc) { g_last_error = "block bounds are defined on the 2-bit planes: the set holds more than four distinct symbols"; return ISOCON_E_ALPHABET; }
    const uint32_t n = s->dev.n;
    if (n >= (1u << 30) || s->maxlen >= 16384) return ISOCON_E_ARG;          // (the list word's 30 index bits, the meta word's 14 length bits)
    for (uint32_t i = 0; i < n; ++i)
        if (thr[i] < 0 || thr[i] > 64) { g_last_error = "threshold outside 0 .. 64"; return ISOCON_E_ARG; }
    // a chunk of the list builder holds 1 .. NN_LIST_CHUNK + 63 pairs: it leaves as soon as a group of 64 row positions has filled the buffer
    // to NN_LIST_CHUNK (nn_surv_core.hpp), and the filter's pass[] holds NN_STAGE
    static_assert(NN_LIST_CHUNK + 63 <= NN_STAGE, "a chunk fits the filter's staging buffer");
    if (chunk_ptr[0] != 0) return ISOCON_E_ARG;
    uint32_t n_narrow = 0;
    for (uint32_t c = 0; c < n_chunks; ++c) {
        if (owner[c] >= n || narrow[c] > 1) { g_last_error = "chunk owner out of range"; return ISOCON_E_ARG; }
        if (chunk_ptr[c + 1] <= chunk_ptr[c] || chunk_ptr[c + 1] - chunk_ptr[c] > NN_LIST_CHUNK + 63) { g_last_error = "chunk count outside 1 .. NN_LIST_CHUNK + 63"; return ISOCON_E_ARG; }
        n_narrow += narrow[c];
    }
    const uint64_t total = chunk_ptr[n_chunks];
    for (uint64_t i = 0; i < total; ++i)
        if ((words[i] & 0x3fffffffu) >= n) { g_last_error = "partner index out of range"; return ISOCON_E_ARG; }
    if (chunks_cap < n_chunks || list_cap < total || pairs_cap < total) { g_last_error = "an output capacity below the worst case (every pair kept)"; return ISOCON_E_ARG; }
    // meta words in the layout of k_nn_entry_meta (no roles, no score: the filter reads the threshold alone); chunk records, wide in front
    const uint64_t cap_in = n_chunks, cap_out = n_chunks;
    const uint64_t tasks_cap = second_pass ? 2 * cap_in + total / 64 + 1 : 0;
    std::vector<uint32_t> meta((size_t)n + NN_META_PAD, 0u);
    for (uint32_t i = 0; i < n; ++i) meta[i] = ((uint32_t)s->lens[i] & 0x3fffu) | ((uint32_t)thr[i] << 14);
    std::vector<NNChunk> chunks(2 * (size_t)cap_in);
    NNPlanTotals tot;
    memset(&tot, 0, sizeof(tot));
    for (uint32_t c = 0; c < n_chunks; ++c) {
        NNChunk ch; ch.slot = owner[c]; ch.count = (uint32_t)(chunk_ptr[c + 1] - chunk_ptr[c]); ch.begin = chunk_ptr[c];
        chunks[narrow[c] ? cap_in + tot.n_chunks_narrow++ : tot.n_chunks++] = ch;
    }
    const uint32_t stride = nnf_text2_stride(s->maxlen);
    DevBuf d_text(&s->pool, SLOT_NN_TEXT2), d_meta(&s->pool, SLOT_NN_LDEST), d_tot(&s->pool, SLOT_NN_LTOT), d_chunks(&s->pool, SLOT_NN_LCHUNKS), d_list(&s->pool, SLOT_NN_LIST),
        d_pa(&s->pool, SLOT_NN_LPA), d_pb(&s->pool, SLOT_NN_LPB), d_tasks(&s->pool, SLOT_NN_LTASKS);
    int rc;
    if ((rc = d_text.alloc((size_t)n * stride * 4)) || (rc = d_meta.upload(meta.data(), meta.size() * 4)) || (rc = d_tot.upload(&tot, sizeof(tot))) ||
        (rc = d_chunks.alloc((size_t)(2 * cap_in + 2 * cap_out) * sizeof(NNChunk))) || (rc = d_list.upload(words, (size_t)total * 4)) || (rc = d_pa.alloc((size_t)total * 4)) ||
        (rc = d_pb.alloc((size_t)total * 4)) || (rc = d_tasks.alloc((size_t)std::max<uint64_t>(tasks_cap, 1) * sizeof(NNFTask))))
        return rc;
    ISO_HIP_CHECK(copy_h2d(d_chunks.p, chunks.data(), chunks.size() * sizeof(NNChunk)));
    NNChunk *left = d_chunks.as<NNChunk>() + 2 * cap_in;
    hipLaunchKernelGGL(k_build_text2, dim3(n), dim3(256), 0, 0, s->dev, d_text.as<uint32_t>(), stride);
    ISO_HIP_CHECK(hipGetLastError());
    ISO_HIP_CHECK(nnf_launch_filter(d_text.as<uint32_t>(), stride, s->dev.lens, d_meta.as<uint32_t>(), kcap, d_list.as<uint32_t>(), d_chunks.as<NNChunk>(), cap_in, left, cap_out,
                                    d_pa.as<uint32_t>(), d_pb.as<uint32_t>(), total, d_tot.as<NNPlanTotals>(), list_min, second_pass ? d_tasks.as<NNFTask>() : (NNFTask *)nullptr,
                                    tasks_cap, NNSeedKnown{nullptr, 0u}));
    ISO_HIP_CHECK(memcpy_wait(&tot, d_tot.p, sizeof(tot), hipMemcpyDeviceToHost));
    const uint64_t counters[9] = {tot.f_chunks, tot.f_chunks_narrow, tot.n_small, tot.f_rejected, tot.f_rejected2, tot.f_listed, tot.f_narrow_listed, tot.f_tasks, tot.overflow};
    for (int i = 0; i < 9; ++i) out_counters[i] = counters[i];
    if (tot.overflow || tot.f_chunks > cap_in - n_narrow || tot.f_chunks_narrow > n_narrow || tot.n_small > total) { g_last_error = "the block filter left more than it was given"; return ISOCON_E_HIP; }
    // the chunks left for the tables, wide then narrow; the list they index; the flat pairs
    std::vector<NNChunk> out((size_t)(tot.f_chunks + tot.f_chunks_narrow));
    if (tot.f_chunks) ISO_HIP_CHECK(copy_d2h(out.data(), left, (size_t)tot.f_chunks * sizeof(NNChunk)));
    if (tot.f_chunks_narrow) ISO_HIP_CHECK(copy_d2h(out.data() + tot.f_chunks, left + cap_out, (size_t)tot.f_chunks_narrow * sizeof(NNChunk)));
    for (size_t i = 0; i < out.size(); ++i) { out_slot[i] = out[i].slot; out_count[i] = out[i].count; out_begin[i] = out[i].begin; }
    ISO_HIP_CHECK(copy_d2h(out_list, d_list.p, (size_t)total * 4));
    if (tot.n_small) {
        ISO_HIP_CHECK(copy_d2h(out_pa, d_pa.p, (size_t)tot.n_small * 4));
        ISO_HIP_CHECK(copy_d2h(out_pb, d_pb.p, (size_t)tot.n_small * 4));
    }
    return ISOCON_OK;
}

// Every isocon_*_last_stats: the first min(cap, count) statistics of the calling thread's last call into out; how many were written.
static int copy_last_stats(const double *stats, int count, double *out, int32_t cap)
{
    if (!out || cap < 0) return 0;
    const int k = cap < count ? cap : count;
    for (int i = 0; i < k; ++i) out[i] = stats[i];
    return k;
}

#include "nn_context.inc"
#include "nn_bounds.inc"
#include "nn_lists.inc"
#include "nn_main.inc"
#include "nn_wide.inc"
#include "nn_images.inc"
#include "nn_entry.inc"
#include "nn2_depth.inc"
#include "sg_host.inc"
#include "msa_host.inc"
#include "hw_host.inc"
#include "hw_loc_host.inc"
#include "hw_full_host.inc"
#include "hw_loc_wide_host.inc"
#include "hw_graph_host.inc"
#include "end_inv_host.inc"
#include "nw_path_host.inc"
#include "hw_path_host.inc"
#include "shw_host.inc"
#include "readtab_host.inc"
#include "edgevar_host.inc"
#include "pbound_host.inc"

extern "C" int isocon_partition_ids(uint32_t n, const int32_t *degree, uint64_t n_edges, const uint32_t *edge_a, const uint32_t *edge_b,
                                    const uint32_t *rank, int32_t nbr_tiebreak, uint32_t *out_centre, int64_t *out_weight,
                                    uint64_t *out_member_ptr, uint32_t *out_members, uint32_t *n_parts)
{
    if (!out_member_ptr || !n_parts || (n && (!degree || !rank || !out_centre || !out_weight || !out_members)) || (n_edges && (!edge_a || !edge_b))) return ISOCON_E_ARG;
    return partition_ids_impl(n, degree, n_edges, edge_a, edge_b, rank, nbr_tiebreak, out_centre, out_weight, out_member_ptr, out_members, n_parts);
}
