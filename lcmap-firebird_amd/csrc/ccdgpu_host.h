// ccdgpu_host.h -- what the host API's units share (ccdgpu_api.cpp: contexts, staging, detection,
// row chain and fetches; ccdgpu_forest.cpp; ccdgpu_train.cpp; ccdgpu_splits.cpp; ccdgpu_predict.cpp; ccdgpu_products.cpp): the owners of device memory,
// pinned memory and events, and the context.  Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>

#include "ccd_products.h"
#include "ccdgpu_checks.h"

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return ccdhost::fail(CCDGPU_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace ccdhost {

// Device memory, grown on demand and freed with its owner.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t n) {
        if (n <= cap && p) return 0;
        release();
        if (hipMalloc(&p, sizeof(T) * (n ? n : 1)) != hipSuccess) {
            p = nullptr;
            return fail(CCDGPU_ENOMEM, "hipMalloc failed (" + std::to_string(sizeof(T) * n) + " bytes)");
        }
        cap = n;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Page-locked host staging (hipHostMalloc), grown on demand: device-to-host copies into it run as
// one DMA at link speed instead of the runtime's chunked bounce through its own pinned buffers.
struct PinBuf {
    unsigned char *p = nullptr;
    size_t cap = 0;  // bytes
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { release(); }
    int ensure(size_t n) {
        if (n <= cap && p) return 0;
        release();
        if (hipHostMalloc(reinterpret_cast<void **>(&p), n ? n : 1, hipHostMallocDefault) != hipSuccess) {
            p = nullptr;
            return fail(CCDGPU_ENOMEM, "hipHostMalloc failed (" + std::to_string(n) + " bytes)");
        }
        cap = n;
        return 0;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// An event destroyed with its owner; create() makes it once (a second call keeps the first).
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

// The forest of the last ccdgpu_forest_train (ccdgpu_train.cpp): the ccdgpu_forest arrays, on the host,
// and the nodes' weighted class counts [n_nodes][n_classes] (the c_k that value is made of).
struct Trained {
    bool has = false;
    int32_t n_features = 0, n_classes = 0;
    std::vector<int32_t> root, feature, left, right;
    std::vector<double> threshold, value;
    std::vector<int64_t> counts;
};

}  // namespace ccdhost

struct ccdgpu_ctx {
    template <class T>
    using DevBuf = ccdhost::DevBuf<T>;
    using PinBuf = ccdhost::PinBuf;
    using Event = ccdhost::Event;
    using Shape = ccdhost::Shape;

    int device = 0;
    int n_cu = 0;
    int slots_per_cu = 0;
    int variant = 4;  // detection kernel register budget: 1..4 waves/SIMD (CCDGPU_KERNEL=w1..w4)
    int poison = 0;   // CCDGPU_POISON=1: LDS and slot scratch filled with NaN bytes per pixel (test mode)
    int arg_slot = -1;  // this context's launch-argument slot in constant memory
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // uploads of ccdgpu_stage_slot (overlap a running detection)
    hipStream_t up_stream = nullptr;    // where the slot uploads go: copy_stream, or the device's shared one
    // every other kernel and copy of a launch (prep, CSR scan and pool -> CSR, row packing, small
    // copies): the detection stream itself, or -- with CUs reserved (ccdgpu_init_copy_cus) -- a
    // stream on the reserved CUs, so these short kernels never wait for wave slots behind
    // persistent detection waves; only the detection kernel then runs on `stream`
    hipStream_t aux = nullptr;
    bool aux_own = false;
    Event uploaded[CCDGPU_UPLOAD_SLOTS];
    // inputs the next detection reads: the single staged batch, or one of the two upload slots
    const int64_t *in_dates = nullptr;
    const int16_t *in_spectra = nullptr;
    const uint16_t *in_qa = nullptr;
    const unsigned char *in_enc = nullptr;  // a transport-encoded batch the kernel reads in place
    // decode encoded uploads into the standard layout first (CCDGPU_DECODE=1: the round-3 path, A/B)
    bool decode_enc = false;
    bool keep_slots = false;  // CCDGPU_KEEP_SLOTS=1 (measurement only, tools/overlap_test.py): a slot stays staged after its run
    Event ev[4];
    // the host waits for a detection through this event: blocking (the waiting thread sleeps on
    // the completion interrupt instead of polling), so the tile driver's waiting workers leave the
    // host's CPUs to its fetch / encode threads
    Event done;
    // staged batch
    bool staged = false, ran = false;
    ccdgpu_params params{};
    Shape shape;
    int32_t mask_words = 0, n_slots = 0;
    int64_t total_pix = 0, pool_cap = 0, n_pool = 0;
    // initial segment-pool room per pixel (CCDGPU_POOL_PER_PIXEL, test knob: a small pool makes
    // every change-dense batch take the overflow rerun) and the reruns of the last run
    int pool_per_pixel = 8;
    int64_t pool_reruns = 0;
    DevBuf<int64_t> dates, sdates, offsets;
    DevBuf<int16_t> spectra;
    DevBuf<uint16_t> qa;
    DevBuf<int32_t> order, procedure, nseg, pool_seq, chip_nobs;
    DevBuf<int64_t> chip_obs_off, chip_pix_off, chip_data_off;
    DevBuf<double> basis, probs, s_f64;
    DevBuf<unsigned long long> counters, stats;
    DevBuf<int32_t> s_date;
    DevBuf<uint16_t> s_row;
    DevBuf<uint16_t> s_bk;
    DevBuf<uint32_t> mask;
    DevBuf<ccdgpu_segment> pool, csr;
    DevBuf<unsigned char> cub_tmp;
    DevBuf<ccdgpu_row> rows;    // output writer scratch (ccdgpu_fetch_rows / ccdgpu_fetch_batch_rows)
    DevBuf<int64_t> row_off, seg_off1;
    DevBuf<int32_t> row_xy;     // per-chip (cx, cy) of a batch row fetch
    DevBuf<int8_t> mask8;
    PinBuf h_rows;              // pinned landing zone of a batch row fetch (rows, then mask words)
    // pinned staging of every launch's small host <-> device copies (initial counters, kernel
    // arguments, counters and statistics read back, CSR offsets): DMA from / to pinned memory,
    // where pageable memory would go through a runtime staging copy -- a blit kernel that has to
    // wait for free CUs while other contexts' detection kernels hold them all
    PinBuf h_small, h_off, h_tab, h_fo, h_xy;  // (h_tab: chip tables of a launch; h_fo: row-fetch offsets)
    DevBuf<int64_t> slot_dates[CCDGPU_UPLOAD_SLOTS];   // upload slots (ccdgpu_stage_slot / ccdgpu_run_slot)
    DevBuf<int16_t> slot_spectra[CCDGPU_UPLOAD_SLOTS];
    DevBuf<uint16_t> slot_qa[CCDGPU_UPLOAD_SLOTS];
    DevBuf<unsigned char> slot_enc[CCDGPU_UPLOAD_SLOTS];  // transport-encoded uploads (ccdgpu_stage_slot_encoded)
    Shape slot_shape[CCDGPU_UPLOAD_SLOTS];
    ccdgpu_params slot_params[CCDGPU_UPLOAD_SLOTS];
    bool slot_ready[CCDGPU_UPLOAD_SLOTS] = {};
    bool slot_encoded[CCDGPU_UPLOAD_SLOTS] = {};  // the slot holds an encoded batch read in place
    DevBuf<unsigned char> b64;  // chipmunk payload text of the last ccdgpu_stage_chipmunk
    DevBuf<int64_t> b64_off;
    std::vector<int64_t> h_offsets;
    ccdgpu_stats last{};
    unsigned long long diag[CCD_NSTATS] = {};
    // a detection launched by ccdgpu_run_slot_begin and not yet finished by ccdgpu_run_slot_end
    bool pending = false;
    int32_t pend_slot = -1;  // the upload slot that detection reads (not to be restaged until it ends)
    CcdDetectArgs pend_args{};
    // the batch chain of ccdgpu_run_slot_begin_rows: CSR, row packing and the copies of rows,
    // row offsets and mask words into the caller's (pinned) buffers, enqueued behind the
    // detection; `done_rows` marks the end of the chain
    bool rows_mode = false;
    int64_t *rq_offsets = nullptr, *rq_seg = nullptr;
    ccdgpu_row *rq_rows = nullptr;
    uint32_t *rq_mask = nullptr;
    int64_t rq_offsets_cap = 0, rq_rows_cap = 0, rq_mask_cap = 0;
    int32_t rq_width = 100;
    std::vector<int32_t> rq_cx, rq_cy;
    DevBuf<int64_t> rowcnt;
    Event done_rows;
    // the context's random forest (ccdgpu_forest_set; ccd_forest.hip) and the scratch of a
    // classification: feature matrix, skip flags, aux values and predictions of a slab of rows
    bool has_forest = false;
    CcdForestDev forest{};
    DevBuf<unsigned char> f_pool, f_skip;
    DevBuf<int64_t> f_tree_off;
    DevBuf<int32_t> f_chunk_first;
    DevBuf<double> f_x, f_aux;
    DevBuf<float> f_out;
    Event f_ev[2];
    // the out-of-bag walk (ccdgpu_forest_oob): the forest's tree count, and per call the trees' hash
    // keys and a slab's counts of scoring trees
    int32_t f_n_trees = 0;
    DevBuf<uint64_t> f_keys;
    DevBuf<int32_t> f_noob;
    // the permutation counts (ccdgpu_forest_permutation; f_x holds the whole matrix for the call): the
    // labels, the columns' (a, b) pairs, and the four counter arrays back to back
    DevBuf<int32_t> f_labels;
    DevBuf<uint32_t> f_ab, f_cnt;
    // the forest trained last (ccdgpu_forest_train); not the context's forest until it is set
    ccdhost::Trained trained;
    // prediction of band values (ccd_predict.hip): pixels whose output the device holds at a time
    // (CCDGPU_PREDICT_SLAB_PIXELS, test knob; 0: as many as keep a slab within PREDICT_SLAB_BYTES)
    // and the scratch of a slab -- dates, basis, offsets, table rows, values, row indices
    int64_t predict_slab_pixels = 0;
    DevBuf<int64_t> p_dates, p_off;
    DevBuf<double> p_basis;
    DevBuf<ccdgpu_row> p_rows;
    DevBuf<unsigned char> p_out;
    DevBuf<int32_t> p_idx;
    Event p_ev[2];
    // product rasters (ccd_products.hip): pixels whose output the device holds at a time
    // (CCDGPU_PRODUCT_SLAB_PIXELS, test knob; 0: as many as keep a slab within PRODUCT_SLAB_BYTES) and
    // the scratch of a slab -- dates with their year windows (and the host copy they are uploaded
    // from), offsets, table rows, rfrawp rows, records, product planes
    int64_t product_slab_pixels = 0;
    std::vector<int64_t> q_win_host;
    DevBuf<int64_t> q_win, q_off;
    DevBuf<ccdgpu_row> q_rows;
    DevBuf<float> q_rf;
    DevBuf<CcdProductRecord> q_rec;
    DevBuf<unsigned char> q_out;
    Event q_ev[2];
    // Buffers and events free themselves (after this body, so after the streams are gone:
    // ccdgpu_destroy has synchronised every stream); here only what has an order or a condition.
    ~ccdgpu_ctx();
};

namespace ccdhost {

// the refusal of every call that may not run while a detection begun with ccdgpu_run_slot_begin
// (or _begin_rows) is pending
int busy(const ccdgpu_ctx *c);

// Segment offsets and row offsets (rows per pixel = max(1, segments)) of pixels [p0, p0 + np) of
// the last run, both relative to the first pixel, from the host's CSR offsets into h_fo
// ([np + 1] int64 each, segment offsets first); *n_rows: their rows.  upload: also to seg_off1 /
// row_off on the aux stream.
int make_row_offsets(ccdgpu_ctx *c, int64_t p0, int64_t np, bool upload, int64_t *n_rows);

}  // namespace ccdhost
