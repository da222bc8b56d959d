// ccdgpu_api.cpp -- host side of the C-ABI declared in include/ccdgpu.h.
//
// Owns device memory and two HIP streams per context.  A detection call = H2D of the chip stacks
// (band-major, observation-contiguous, exactly the layout the Python packer hands over; chips of
// different observation counts packed back to back), the per-chip prep kernel, the persistent
// per-pixel detection kernel, an exclusive scan of the per-pixel segment counts (hipCUB) and the
// pool->CSR scatter, then D2H of the CSR result or of the device-packed table rows.
// Replaces the per-pixel ccd.detect call of ccdc/pyccd.py:168 (see include/ccdgpu.h).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <chrono>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ccdgpu.h"
#include "ccd_device.h"
#include "ccd_enc_layout.h"
#include "ccd_predict.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(CCDGPU_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;  // elements
    int ensure(size_t n) {
        if (n <= cap && p) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
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
    int ensure(size_t n) {
        if (n <= cap && p) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
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

double chi2_5_cdf(double x) {
    if (x <= 0) return 0.0;
    return std::erf(std::sqrt(x / 2.0)) - std::sqrt(2.0 * x / M_PI) * std::exp(-x / 2.0) * (1.0 + x / 3.0);
}

// inverse chi-square(5) cdf (change.adjustchgthresh uses scipy chi2.ppf(pt_cg, 5))
double chi2_5_ppf(double p) {
    double lo = 0.0, hi = 400.0;
    for (int i = 0; i < 200; ++i) {
        const double mid = 0.5 * (lo + hi);
        if (chi2_5_cdf(mid) < p) lo = mid;
        else hi = mid;
    }
    return 0.5 * (lo + hi);
}

// constant-memory launch-argument slots (CCD_ARG_SLOTS per process): one per live context
std::mutex g_slot_mu;
unsigned g_slots_used = 0;
int acquire_arg_slot() {
    std::lock_guard<std::mutex> g(g_slot_mu);
    for (int i = 0; i < CCD_ARG_SLOTS; ++i)
        if (!(g_slots_used & (1u << i))) {
            g_slots_used |= 1u << i;
            return i;
        }
    return -1;
}
void release_arg_slot(int i) {
    if (i < 0) return;
    std::lock_guard<std::mutex> g(g_slot_mu);
    g_slots_used &= ~(1u << i);
}

// Shape of a staged batch: per-chip pixel / observation counts and their prefix sums
// (ccd_device.h layout).
struct Shape {
    std::vector<int32_t> npix, nobs;
    std::vector<int64_t> obs_off, pix_off, data_off;  // [n_chips + 1]
    int32_t n_obs_max = 0;
    int n_chips() const { return (int)npix.size(); }
    int64_t total_obs() const { return obs_off.empty() ? 0 : obs_off.back(); }
    int64_t total_pix() const { return pix_off.empty() ? 0 : pix_off.back(); }
    int64_t total_data() const { return data_off.empty() ? 0 : data_off.back(); }
};

int make_shape(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs, Shape &s) {
    if (n_chips <= 0) return fail(CCDGPU_EINVAL, "n_chips must be > 0");
    if (!n_pix || !n_obs) return fail(CCDGPU_EINVAL, "NULL n_pix / n_obs array");
    s.npix.assign(n_pix, n_pix + n_chips);
    s.nobs.assign(n_obs, n_obs + n_chips);
    s.obs_off.assign(n_chips + 1, 0);
    s.pix_off.assign(n_chips + 1, 0);
    s.data_off.assign(n_chips + 1, 0);
    s.n_obs_max = 0;
    for (int c = 0; c < n_chips; ++c) {
        if (n_pix[c] <= 0) return fail(CCDGPU_EINVAL, "chip " + std::to_string(c) + ": n_pix must be > 0");
        if (n_obs[c] <= 0 || n_obs[c] > CCDGPU_MAX_OBS)
            return fail(CCDGPU_EINVAL, "chip " + std::to_string(c) + ": n_obs must be in [1, " + std::to_string(CCDGPU_MAX_OBS) + "]");
        s.obs_off[c + 1] = s.obs_off[c] + n_obs[c];
        s.pix_off[c + 1] = s.pix_off[c] + n_pix[c];
        s.data_off[c + 1] = s.data_off[c] + (int64_t)n_pix[c] * n_obs[c];
        s.n_obs_max = std::max(s.n_obs_max, n_obs[c]);
    }
    if (s.total_pix() >= (int64_t)1 << 31) return fail(CCDGPU_EINVAL, "more than 2^31 - 1 pixels in one batch");
    return 0;
}

// One upload stream per device shared by every context (unless CCDGPU_SHARED_UPLOADS=0):
// the host-to-device copies of all contexts then run one after another in the order they were
// staged -- the order their detections need them -- instead of side by side on separate DMA
// queues, where every upload in flight shares the link and each finishes late.  Created on first
// use, kept for the process's lifetime.
std::mutex g_up_mu;
hipStream_t g_up_stream[64] = {};
hipStream_t shared_upload_stream(int device) {
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> g(g_up_mu);
    if (!g_up_stream[device] && hipStreamCreateWithFlags(&g_up_stream[device], hipStreamNonBlocking) != hipSuccess)
        g_up_stream[device] = nullptr;
    return g_up_stream[device];
}

}  // namespace

struct ccdgpu_ctx {
    int device = 0;
    int n_cu = 0;
    int slots_per_cu = 0;
    int variant = 4;  // detection kernel register budget: 1..4 waves/SIMD (CCDGPU_KERNEL=w1..w4)
    int poison = 0;   // CCDGPU_POISON=1: LDS and slot scratch filled with NaN bytes per pixel (test mode)
    int arg_slot = -1;  // this context's launch-argument slot in constant memory
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // uploads of ccdgpu_stage_slot (overlap a running detection)
    hipStream_t up_stream = nullptr;    // where the slot uploads go: copy_stream, or the device's shared one
    // every other kernel and copy of a launch (prep, CSR scan and scatter, row packing, small
    // copies): the detection stream itself, or -- with CUs reserved (ccdgpu_init_copy_cus) -- a
    // stream on the reserved CUs, so these short kernels never wait for wave slots behind
    // persistent detection waves; only the detection kernel then runs on `stream`
    hipStream_t aux = nullptr;
    bool aux_own = false;
    hipEvent_t uploaded[CCDGPU_UPLOAD_SLOTS] = {};
    // inputs the next detection reads: the single staged batch, or one of the two upload slots
    const int64_t *in_dates = nullptr;
    const int16_t *in_spectra = nullptr;
    const uint16_t *in_qa = nullptr;
    const unsigned char *in_enc = nullptr;  // a transport-encoded batch the kernel reads in place
    // decode encoded uploads into the standard layout first (CCDGPU_DECODE=1: the round-3 path, A/B)
    bool decode_enc = false;
    bool rows_fused = true;   // CCDGPU_ROWS_FUSED=0 (A/B): the separate scatter and per-chip row packing
    bool keep_slots = false;  // CCDGPU_KEEP_SLOTS=1 (measurement only, tools/overlap_test.py): a slot stays staged after its run
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // the host waits for a detection through this event: blocking (the waiting thread sleeps on
    // the completion interrupt instead of polling), so the tile driver's waiting workers leave the
    // host's CPUs to its fetch / encode threads
    hipEvent_t done = nullptr;
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
    hipEvent_t done_rows = nullptr;
    // the context's random forest (ccdgpu_forest_set; ccd_forest.hip) and the scratch of a
    // classification: feature matrix, skip flags, aux values and predictions of a slab of rows
    bool has_forest = false;
    CcdForestDev forest{};
    DevBuf<unsigned char> f_pool, f_skip;
    DevBuf<int64_t> f_tree_off;
    DevBuf<int32_t> f_chunk_first;
    DevBuf<double> f_x, f_aux;
    DevBuf<float> f_out;
    hipEvent_t f_ev[2] = {nullptr, nullptr};
    // prediction of band values (ccd_predict.hip): pixels whose output the device holds at a time
    // (CCDGPU_PREDICT_SLAB_PIXELS, test knob; 0: as many as keep a slab within PREDICT_SLAB_BYTES)
    // and the scratch of a slab -- dates, basis, offsets, table rows, values, row indices
    int64_t predict_slab_pixels = 0;
    DevBuf<int64_t> p_dates, p_off;
    DevBuf<double> p_basis;
    DevBuf<ccdgpu_row> p_rows;
    DevBuf<unsigned char> p_out;
    DevBuf<int32_t> p_idx;
    hipEvent_t p_ev[2] = {nullptr, nullptr};
    ~ccdgpu_ctx() {
        for (auto *b : {&dates, &sdates, &offsets, &chip_obs_off, &chip_pix_off, &chip_data_off, &row_off, &seg_off1, &b64_off})
            b->release();
        spectra.release();
        qa.release();
        for (auto *b : {&order, &procedure, &nseg, &pool_seq, &s_date, &chip_nobs, &row_xy}) b->release();
        for (auto *b : {&basis, &probs, &s_f64}) b->release();
        counters.release();
        stats.release();
        s_row.release();
        s_bk.release();
        mask.release();
        pool.release();
        csr.release();
        cub_tmp.release();
        b64.release();
        for (int i = 0; i < CCDGPU_UPLOAD_SLOTS; ++i) {
            slot_dates[i].release();
            slot_spectra[i].release();
            slot_qa[i].release();
            slot_enc[i].release();
            if (uploaded[i]) (void)hipEventDestroy(uploaded[i]);
        }
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        rows.release();
        mask8.release();
        h_rows.release();
        h_small.release();
        h_off.release();
        h_tab.release();
        h_fo.release();
        h_xy.release();
        if (aux_own && aux) (void)hipStreamDestroy(aux);
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
        if (done) (void)hipEventDestroy(done);
        if (done_rows) (void)hipEventDestroy(done_rows);
        rowcnt.release();
        f_pool.release();
        f_skip.release();
        f_tree_off.release();
        f_chunk_first.release();
        f_x.release();
        f_aux.release();
        f_out.release();
        for (auto &e : f_ev)
            if (e) (void)hipEventDestroy(e);
        p_dates.release();
        p_off.release();
        p_basis.release();
        p_rows.release();
        p_out.release();
        p_idx.release();
        for (auto &e : p_ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
        release_arg_slot(arg_slot);
    }
};

extern "C" {

const char *ccdgpu_version(void) { return "ccdgpu 0.2.0 (gfx950; lcmap-pyccd:2018.03.12.dev-ncompare.b2 semantics)"; }

const char *ccdgpu_last_error(void) { return g_err.c_str(); }

void ccdgpu_params_default(ccdgpu_params *p) {
    std::memset(p, 0, sizeof(*p));
    p->meow_size = 12;
    p->peek_size = 6;
    p->day_delta = 365;
    p->coef_min = 4;
    p->coef_mid = 6;
    p->coef_max = 8;
    p->num_obs_factor = 3;
    p->detection_bands = 0x3E;
    p->tmask_bands = 0x12;
    p->lasso_max_iter = 1000;
    p->thermal_min = -9320;
    p->thermal_max = 7070;
    p->median_green_filter = 400;
    p->curve_qa_start = 14;
    p->curve_qa_end = 24;
    p->curve_qa_insuf_clear = 44;
    p->curve_qa_persist_snow = 54;
    p->qa_fill = 0;
    p->qa_clear = 1;
    p->qa_water = 2;
    p->qa_shadow = 3;
    p->qa_snow = 4;
    p->qa_cloud = 5;
    p->qa_cirrus1 = 8;
    p->qa_cirrus2 = 9;
    p->qa_occlusion = 10;
    p->qa_bitpacked = 1;
    p->adaptive_peek = 1;
    p->rmse_dof = 0;
    p->kelvin_to_celsius = 1;
    p->avg_days_yr = 365.2425;
    p->change_probability = 0.99;
    p->change_threshold = 15.086272469388987;
    p->outlier_threshold = 35.888186879610423;
    p->t_const = 4.42;
    p->lasso_alpha = 1.0;
    p->lasso_tol = 1e-4;
    p->clear_pct_threshold = 0.25;
    p->snow_pct_threshold = 0.75;
    p->argsort_stable = 0;  // numpy quicksort tie order (include/ccdgpu.h)
    p->reserved0 = 0;
}

int ccdgpu_device_count(int *count) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *count = 0;
        return fail(CCDGPU_EHIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = c;
    return 0;
}

int ccdgpu_device_numa_node(int device, int *node) {
    if (!node) return fail(CCDGPU_EINVAL, "node out pointer is NULL");
    *node = -1;
    char bus[64] = {0};
    HIPCHK(hipDeviceGetPCIBusId(bus, (int)sizeof(bus) - 1, device));
    for (char *q = bus; *q; ++q) *q = (char)std::tolower((unsigned char)*q);
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
    FILE *f = std::fopen(path.c_str(), "r");
    if (!f) return 0;  // not exposed: unknown
    int v = -1;
    if (std::fscanf(f, "%d", &v) != 1) v = -1;
    std::fclose(f);
    *node = v;
    return 0;
}

int ccdgpu_init(int device, ccdgpu_ctx **out) { return ccdgpu_init_copy_cus(device, 0, out); }

int ccdgpu_init_copy_cus(int device, int copy_cus, ccdgpu_ctx **out) {
    if (!out) return fail(CCDGPU_EINVAL, "ctx out pointer is NULL");
    if (copy_cus < 0) return fail(CCDGPU_EINVAL, "copy_cus must be >= 0");
    *out = nullptr;
    int count = 0;
    int rc = ccdgpu_device_count(&count);
    if (rc) return rc;
    if (device < 0 || device >= count)
        return fail(CCDGPU_EINVAL, "device " + std::to_string(device) + " out of range (" + std::to_string(count) + " visible)");
    HIPCHK(hipSetDevice(device));
    auto *c = new ccdgpu_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        delete c;
        return fail(CCDGPU_EHIP, "hipGetDeviceProperties failed");
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::string arch = prop.gcnArchName;
        delete c;
        return fail(CCDGPU_EHIP, "device " + std::to_string(device) + " is " + arch + ", libccdgpu is built for gfx950 only");
    }
    c->n_cu = prop.multiProcessorCount;
    // copy_cus = k > 0: the copy stream (uploads' decode kernel, blits) gets k CUs of its own --
    // the same k for every context -- and the detection stream the rest, so a context's upload is
    // never starved of CUs by other contexts' persistent detection waves (which otherwise hold
    // every wave slot until their launch drains).  The mask bits are the last ceil(k / 8) of each
    // run of n_cu / 8.  The driver maps mask bit i to XCD i % 8 (the i / 8-th CU of that XCD,
    // shader engines interleaved; tools/probe/cu_mask.hip, profiles/r04/cu_mask_probe.txt), so for
    // k = 8 these are one shader engine of XCD 7: the detection stream runs on the other 248 CUs,
    // and the copy / aux streams -- whose masks are empty on XCDs 0-6, which the hardware treats
    // as unrestricted -- have those 8 CUs to themselves and share the rest.  The truly
    // interleaved reservation (ceil(k / 8) CUs on every XCD and nothing else for the copy
    // streams, CCDGPU_MASK_INTERLEAVED=1) measured slower: one context's detection 2.29M vs
    // 2.44M px/s (the same as with no reservation), four contexts with the batch chain 2.62M vs
    // 2.72M (profiles/r04/cu_layout_ab.txt).  CCDGPU_COPY_CUS overrides k (experiments).
    if (const char *e = std::getenv("CCDGPU_COPY_CUS")) copy_cus = std::max(0, std::atoi(e));
    const char *mi = std::getenv("CCDGPU_MASK_INTERLEAVED");
    const bool blocked = !(mi && std::atoi(mi) != 0);
    std::vector<uint32_t> mask_det, mask_copy;
    if (copy_cus > 0 && copy_cus < c->n_cu) {
        const int nw = (c->n_cu + 31) / 32, groups = 8, per = c->n_cu / groups;
        // at least one CU of every group stays with the detection stream, and at least one is reserved
        const int k = std::min((copy_cus + groups - 1) / groups, per - 1);
        if (per < 2 || k < 1) {
            const std::string msg = "copy_cus " + std::to_string(copy_cus) + " leaves no CU for detection or copies on " +
                                    std::to_string(c->n_cu) + " CUs";
            delete c;
            return fail(CCDGPU_EINVAL, msg);
        }
        mask_det.assign(nw, 0u);
        mask_copy.assign(nw, 0u);
        for (int cu = 0; cu < c->n_cu; ++cu) {
            const bool reserved = blocked ? (cu % per) >= per - k : cu >= c->n_cu - groups * k;
            (reserved ? mask_copy : mask_det)[cu / 32] |= 1u << (cu % 32);
        }
    }
    const bool masked = !mask_det.empty();
    if ((masked ? hipExtStreamCreateWithCUMask(&c->stream, (uint32_t)mask_det.size(), mask_det.data())
                : hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        delete c;
        return fail(CCDGPU_EHIP, "hipStreamCreate failed");
    }
    for (auto &e : c->ev) (void)hipEventCreate(&e);
    (void)hipEventCreateWithFlags(&c->done, hipEventBlockingSync | hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&c->done_rows, hipEventBlockingSync | hipEventDisableTiming);
    if ((masked ? hipExtStreamCreateWithCUMask(&c->copy_stream, (uint32_t)mask_copy.size(), mask_copy.data())
                : hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking)) != hipSuccess) {
        delete c;
        return fail(CCDGPU_EHIP, "hipStreamCreate failed");
    }
    for (auto &e : c->uploaded) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    // uploads in staging order on the device's shared stream (default; CCDGPU_SHARED_UPLOADS=0:
    // each context's own copy stream).  Tile leg A/B: 2.50 / 2.62M vs 2.42 / 2.50M px/s
    // (profiles/r04/tile_knobs.json).
    c->up_stream = c->copy_stream;
    {
        const char *v = std::getenv("CCDGPU_SHARED_UPLOADS");
        if (!v || std::atoi(v) != 0) {
            hipStream_t sh = shared_upload_stream(device);
            if (sh) c->up_stream = sh;
        }
    }
    c->aux = c->stream;
    if (masked) {
        if (hipExtStreamCreateWithCUMask(&c->aux, (uint32_t)mask_copy.size(), mask_copy.data()) != hipSuccess) {
            c->aux = nullptr;
            delete c;
            return fail(CCDGPU_EHIP, "hipStreamCreate failed");
        }
        c->aux_own = true;
    } else if (const char *v = std::getenv("CCDGPU_AUX_PRIORITY")) {
        // no CUs reserved: the launch's other kernels on a high-priority stream of their own, so the
        // dispatcher serves them ahead of waiting detection waves (experiment knob)
        if (std::atoi(v) != 0) {
            int lo = 0, hi = 0;
            if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess &&
                hipStreamCreateWithPriority(&c->aux, hipStreamNonBlocking, hi) == hipSuccess)
                c->aux_own = true;
            else
                c->aux = c->stream;
        }
    }
    c->arg_slot = acquire_arg_slot();
    if (c->arg_slot < 0) {
        delete c;
        return fail(CCDGPU_EINVAL, "more than " + std::to_string(CCD_ARG_SLOTS) + " live contexts in this process");
    }
    c->slots_per_cu = 16;
    c->variant = 4;
    if (const char *v = std::getenv("CCDGPU_KERNEL")) {
        if (v[0] == 'w' && v[1] >= '1' && v[1] <= '4' && v[2] == 0) c->variant = v[1] - '0';
    }
    if (const char *v = std::getenv("CCDGPU_SLOTS_PER_CU")) c->slots_per_cu = std::max(1, std::atoi(v));
    if (const char *v = std::getenv("CCDGPU_POISON")) c->poison = std::atoi(v) != 0;
    if (const char *v = std::getenv("CCDGPU_DECODE")) c->decode_enc = std::atoi(v) != 0;
    if (const char *v = std::getenv("CCDGPU_ROWS_FUSED")) c->rows_fused = std::atoi(v) != 0;
    if (const char *v = std::getenv("CCDGPU_KEEP_SLOTS")) c->keep_slots = std::atoi(v) != 0;
    if (const char *v = std::getenv("CCDGPU_POOL_PER_PIXEL")) c->pool_per_pixel = std::max(1, std::atoi(v));
    if (const char *v = std::getenv("CCDGPU_PREDICT_SLAB_PIXELS")) c->predict_slab_pixels = std::max(0, std::atoi(v));
    *out = c;
    return 0;
}

int ccdgpu_destroy(ccdgpu_ctx *ctx) {
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamSynchronize(ctx->copy_stream);
    if (ctx->up_stream && ctx->up_stream != ctx->copy_stream) (void)hipStreamSynchronize(ctx->up_stream);
    if (ctx->aux) (void)hipStreamSynchronize(ctx->aux);
    delete ctx;
    return 0;
}

int ccdgpu_synchronize(ccdgpu_ctx *ctx) {
    if (!ctx) return fail(CCDGPU_EINVAL, "NULL ctx");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

static int check_params(const ccdgpu_params *p) {
    if (!p) return fail(CCDGPU_EINVAL, "params is NULL");
    if (p->peek_size < 1 || p->peek_size > CCDGPU_MAX_PEEK)
        return fail(CCDGPU_EINVAL, "peek_size must be in [1, " + std::to_string(CCDGPU_MAX_PEEK) + "]");
    if (p->meow_size < 5) return fail(CCDGPU_EINVAL, "meow_size must be >= 5 (Tmask needs > 4 observations)");
    if (p->coef_min != 4 && p->coef_min != 6 && p->coef_min != 8)
        return fail(CCDGPU_EINVAL, "coefficient counts must be 4, 6 or 8");
    if ((p->coef_mid != 4 && p->coef_mid != 6 && p->coef_mid != 8) || (p->coef_max != 4 && p->coef_max != 6 && p->coef_max != 8))
        return fail(CCDGPU_EINVAL, "coefficient counts must be 4, 6 or 8");
    if (p->lasso_max_iter < 1) return fail(CCDGPU_EINVAL, "lasso_max_iter must be >= 1");
    if ((p->detection_bands & ~0x7Fu) || (p->tmask_bands & ~0x7Fu))
        return fail(CCDGPU_EINVAL, "band masks must only use bits 0..6");
    if (p->argsort_stable != 0 && p->argsort_stable != 1) return fail(CCDGPU_EINVAL, "argsort_stable must be 0 or 1");
    return 0;
}

// Device buffers of a staged batch (chip tables, per-slot scratch, outputs) and, with
// base_inputs, the input buffers plus the dates upload; the pixel data are filled by the caller
// (a plain upload or the chipmunk decoder).
static int stage_alloc(ccdgpu_ctx *c, const ccdgpu_params *params, const Shape &sh, const int64_t *dates,
                       bool base_inputs = true) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    int rc = check_params(params);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    c->staged = false;
    c->params = *params;
    c->shape = sh;
    const int nc = sh.n_chips();
    c->mask_words = (sh.n_obs_max + 31) / 32;
    c->total_pix = sh.total_pix();
    const size_t tobs = (size_t)sh.total_obs(), tdata = (size_t)sh.total_data();
    if (base_inputs && ((rc = c->dates.ensure(tobs)) || (rc = c->spectra.ensure(7 * tdata)) || (rc = c->qa.ensure(tdata))))
        return rc;
    if ((rc = c->order.ensure(tobs)) || (rc = c->sdates.ensure(tobs)) || (rc = c->basis.ensure(tobs * CCD_BASIS_STRIDE)) ||
        (rc = c->chip_nobs.ensure(nc)) || (rc = c->chip_obs_off.ensure(nc + 1)) || (rc = c->chip_pix_off.ensure(nc + 1)) ||
        (rc = c->chip_data_off.ensure(nc + 1)) ||
        (rc = c->procedure.ensure(c->total_pix)) || (rc = c->nseg.ensure(c->total_pix)) ||
        (rc = c->probs.ensure(3 * c->total_pix)) || (rc = c->offsets.ensure(c->total_pix + 1)) ||
        (rc = c->mask.ensure((size_t)c->total_pix * c->mask_words)) || (rc = c->counters.ensure(8)) ||
        (rc = c->stats.ensure(CCD_NSTATS)))
        return rc;
    // persistent grid: one wave slot per resident wave (LDS / register occupancy), capped by
    // CCDGPU_SLOTS_PER_CU
    const int occ = ccdk_occupancy(c->variant, sh.n_obs_max);
    if (occ <= 0) return fail(CCDGPU_EHIP, "detection kernel cannot be resident with " + std::to_string(ccdk_lds_bytes(sh.n_obs_max)) + " B of LDS");
    c->n_slots = (int32_t)std::min<int64_t>(c->total_pix, (int64_t)c->n_cu * std::min(occ, c->slots_per_cu));
    const size_t ns = (size_t)c->n_slots, no = (size_t)sh.n_obs_max;
    const size_t nper = ns * no;  // the compacted periods (dates, 16-byte rows) per slot
    if ((rc = c->s_date.ensure(nper)) || (rc = c->s_row.ensure(nper * 8)) ||
        (rc = c->s_f64.ensure(ns * CCD_SLOT_F64(no))) || (rc = c->s_bk.ensure(ns * no)))
        return rc;
    if (c->pool_cap < c->total_pix * c->pool_per_pixel) c->pool_cap = c->total_pix * c->pool_per_pixel;
    c->pool_reruns = 0;
    if ((rc = c->pool.ensure(c->pool_cap)) || (rc = c->pool_seq.ensure(c->pool_cap))) return rc;
    // chip tables, through the context's pinned staging (DMA, no runtime staging copy), on the
    // aux stream that runs the launch's prep; the previous launch's table copies are done
    HIPCHK(hipStreamSynchronize(c->aux));
    const size_t t8 = 8 * ((size_t)nc + 1);
    if ((rc = c->h_tab.ensure(3 * t8 + 4 * (size_t)nc))) return rc;
    unsigned char *ht = c->h_tab.p;
    std::memcpy(ht, sh.obs_off.data(), t8);
    std::memcpy(ht + t8, sh.pix_off.data(), t8);
    std::memcpy(ht + 2 * t8, sh.data_off.data(), t8);
    std::memcpy(ht + 3 * t8, sh.nobs.data(), 4 * (size_t)nc);
    HIPCHK(hipMemcpyAsync(c->chip_obs_off.p, ht, t8, hipMemcpyHostToDevice, c->aux));
    HIPCHK(hipMemcpyAsync(c->chip_pix_off.p, ht + t8, t8, hipMemcpyHostToDevice, c->aux));
    HIPCHK(hipMemcpyAsync(c->chip_data_off.p, ht + 2 * t8, t8, hipMemcpyHostToDevice, c->aux));
    HIPCHK(hipMemcpyAsync(c->chip_nobs.p, ht + 3 * t8, 4 * (size_t)nc, hipMemcpyHostToDevice, c->aux));
    if (dates) HIPCHK(hipMemcpyAsync(c->dates.p, dates, sizeof(int64_t) * tobs, hipMemcpyHostToDevice, c->aux));
    c->in_dates = c->dates.p;
    c->in_spectra = c->spectra.p;
    c->in_qa = c->qa.p;
    c->in_enc = nullptr;
    return 0;
}

static void uniform(int32_t n_chips, int32_t n_pix, int32_t n_obs, std::vector<int32_t> &np, std::vector<int32_t> &no) {
    np.assign(n_chips > 0 ? n_chips : 0, n_pix);
    no.assign(n_chips > 0 ? n_chips : 0, n_obs);
}

int ccdgpu_stage_chips(ccdgpu_ctx *c, const ccdgpu_params *params, int32_t n_chips, const int32_t *n_pix,
                       const int32_t *n_obs, const int64_t *dates, const int16_t *spectra, const uint16_t *qa) {
    if (!dates || !spectra || !qa) return fail(CCDGPU_EINVAL, "NULL input buffer");
    Shape sh;
    int rc = make_shape(n_chips, n_pix, n_obs, sh);
    if (rc) return rc;
    if ((rc = stage_alloc(c, params, sh, dates))) return rc;
    const size_t tdata = (size_t)sh.total_data();
    HIPCHK(hipMemcpyAsync(c->spectra.p, spectra, sizeof(int16_t) * 7 * tdata, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->qa.p, qa, sizeof(uint16_t) * tdata, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->staged = true;
    c->ran = false;
    return 0;
}

int ccdgpu_stage(ccdgpu_ctx *c, const ccdgpu_params *params, int32_t n_chips, int32_t n_pix, int32_t n_obs,
                 const int64_t *dates, const int16_t *spectra, const uint16_t *qa) {
    std::vector<int32_t> np, no;
    uniform(n_chips, n_pix, n_obs, np, no);
    return ccdgpu_stage_chips(c, params, n_chips, np.data(), no.data(), dates, spectra, qa);
}

int ccdgpu_stage_chipmunk(ccdgpu_ctx *c, const ccdgpu_params *params, int32_t n_chips, int32_t n_pix, int32_t n_obs,
                          const int64_t *dates, const char *text, int64_t text_bytes, const int64_t *text_offsets,
                          double *unpack_seconds) {
    if (!dates || !text || !text_offsets || text_bytes < 0) return fail(CCDGPU_EINVAL, "NULL or empty chipmunk text");
    if (n_pix <= 0 || n_pix > (1 << 24)) return fail(CCDGPU_EINVAL, "n_pix out of range");
    if (n_chips <= 0 || n_obs <= 0) return fail(CCDGPU_EINVAL, "n_chips and n_obs must be > 0");
    // Every present payload is exactly the encoded length of n_pix 16-bit values ('=' padded):
    // it must lie inside the text and must not run into the next payload (a truncated payload
    // would otherwise decode its successor's characters as its own tail).
    const int64_t enc = 4 * (((int64_t)2 * n_pix + 2) / 3);
    const int64_t n_off = (int64_t)n_chips * n_obs * 8;
    std::vector<std::pair<int64_t, int64_t>> present;
    present.reserve((size_t)n_off);
    for (int64_t i = 0; i < n_off; ++i) {
        const int64_t o = text_offsets[i];
        if (o < 0) continue;
        if (o + enc > text_bytes)
            return fail(CCDGPU_EINVAL, "chipmunk payload " + std::to_string(i) + " runs past the end of the text");
        present.emplace_back(o, i);
    }
    std::sort(present.begin(), present.end());
    for (size_t k = 0; k + 1 < present.size(); ++k)
        if (present[k + 1].first - present[k].first < enc)
            return fail(CCDGPU_EINVAL, "chipmunk payload " + std::to_string(present[k].second) + " is shorter than " +
                                           std::to_string(enc) + " bytes (" + std::to_string(n_pix) + " values)");
    std::vector<int32_t> np, no;
    uniform(n_chips, n_pix, n_obs, np, no);
    Shape sh;
    int rc = make_shape(n_chips, np.data(), no.data(), sh);
    if (rc) return rc;
    if ((rc = stage_alloc(c, params, sh, dates))) return rc;
    if ((rc = c->b64.ensure((size_t)text_bytes + 8)) || (rc = c->b64_off.ensure((size_t)n_off))) return rc;
    HIPCHK(hipMemcpyAsync(c->b64.p, text, (size_t)text_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->b64_off.p, text_offsets, sizeof(int64_t) * (size_t)n_off, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(c->counters.p, 0, sizeof(unsigned long long) * 8, c->stream));
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    if (ccdk_unpack_b64(c->b64.p, text_bytes, c->b64_off.p, n_chips, n_obs, n_pix, c->spectra.p, c->qa.p,
                        c->counters.p + 5, c->stream))
        return fail(CCDGPU_EHIP, std::string("unpack launch: ") + hipGetErrorString(hipGetLastError()));
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    unsigned long long err = 0;
    HIPCHK(hipMemcpyAsync(&err, c->counters.p + 5, sizeof(err), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
    if (unpack_seconds) *unpack_seconds = ms * 1e-3;
    if (err) return fail(CCDGPU_EINVAL, "chipmunk payload is not valid base64");
    c->staged = true;
    c->ran = false;
    return 0;
}

int ccdgpu_host_alloc(size_t bytes, void **ptr) {
    if (!ptr) return fail(CCDGPU_EINVAL, "NULL ptr");
    *ptr = nullptr;
    if (hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        *ptr = nullptr;
        return fail(CCDGPU_ENOMEM, "hipHostMalloc failed (" + std::to_string(bytes) + " bytes)");
    }
    return 0;
}

int ccdgpu_host_free(void *ptr) {
    if (ptr) HIPCHK(hipHostFree(ptr));
    return 0;
}

int ccdgpu_stage_slot_chips(ccdgpu_ctx *c, int32_t slot, const ccdgpu_params *params, int32_t n_chips,
                            const int32_t *n_pix, const int32_t *n_obs, const int64_t *dates, const int16_t *spectra,
                            const uint16_t *qa) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (slot < 0 || slot >= CCDGPU_UPLOAD_SLOTS)
        return fail(CCDGPU_EINVAL, "slot must be in 0 .. " + std::to_string(CCDGPU_UPLOAD_SLOTS - 1));
    if (c->pending && slot == c->pend_slot)
        return fail(CCDGPU_EINVAL, "slot " + std::to_string(slot) + " is read by the detection begun with ccdgpu_run_slot_begin");
    if (!dates || !spectra || !qa) return fail(CCDGPU_EINVAL, "NULL input buffer");
    Shape sh;
    int rc = make_shape(n_chips, n_pix, n_obs, sh);
    if (rc || (rc = check_params(params))) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t tobs = (size_t)sh.total_obs(), tdata = (size_t)sh.total_data();
    if ((rc = c->slot_dates[slot].ensure(tobs)) || (rc = c->slot_spectra[slot].ensure(7 * tdata)) ||
        (rc = c->slot_qa[slot].ensure(tdata)))
        return rc;
    // the slot's previous batch was detected by a ccdgpu_run_slot that has returned, so the
    // uploads may overwrite it; they run on the copy stream, concurrent with any detection
    HIPCHK(hipMemcpyAsync(c->slot_dates[slot].p, dates, sizeof(int64_t) * tobs, hipMemcpyHostToDevice, c->up_stream));
    HIPCHK(hipMemcpyAsync(c->slot_spectra[slot].p, spectra, sizeof(int16_t) * 7 * tdata, hipMemcpyHostToDevice, c->up_stream));
    HIPCHK(hipMemcpyAsync(c->slot_qa[slot].p, qa, sizeof(uint16_t) * tdata, hipMemcpyHostToDevice, c->up_stream));
    HIPCHK(hipEventRecord(c->uploaded[slot], c->up_stream));
    c->slot_shape[slot] = sh;
    c->slot_params[slot] = *params;  // each slot keeps its own parameters
    c->slot_ready[slot] = true;
    c->slot_encoded[slot] = false;
    return 0;
}

// "encoded batch: chip N" + what is wrong with it
static int enc_fail(int32_t chip, const std::string &what) {
    return fail(CCDGPU_EINVAL, "encoded batch: chip " + std::to_string(chip) + what);
}

// the kept-offset table of a mode 1 or 2 section: a run of at most n_obs per pixel, ending at kept
static int enc_check_koff(int32_t chip, const uint32_t *koff, int64_t n_pix, int64_t n_obs, int64_t kept) {
    if (koff[0] != 0 || (int64_t)koff[n_pix] != kept) return enc_fail(chip, " kept-offset table does not end at kept");
    for (int64_t q = 0; q < n_pix; ++q)
        if (koff[q + 1] < koff[q] || (int64_t)(koff[q + 1] - koff[q]) > n_obs)
            return enc_fail(chip, " kept-offset table is not a run per pixel");
    return 0;
}

// ccdgpu_encoded_check (layout: ccd_enc_layout.h); *packed: the batch holds a mode 2 section (it
// goes to ccd_decode_pack)
static int encoded_check(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs, const uint8_t *enc,
                         int64_t enc_bytes, bool *packed) {
    *packed = false;
    bool mode1 = false;
    if (!enc || !n_pix || !n_obs || n_chips <= 0) return fail(CCDGPU_EINVAL, "NULL or empty encoded batch");
    // the encoded batch must describe exactly these chips (the decoder trusts its headers)
    if (enc_bytes < ccd_enc_table_used(n_chips) || ccd_enc_n_chips(enc) != n_chips)
        return fail(CCDGPU_EINVAL, "encoded batch: chip table does not match n_chips");
    const int64_t *off = ccd_enc_chip_off(enc), *pixo = ccd_enc_chip_pix(enc, n_chips);
    if (off[n_chips] > enc_bytes) return fail(CCDGPU_EINVAL, "encoded batch: longer than enc_bytes");
    int64_t pb = 0, db = 0;
    for (int32_t k = 0; k < n_chips; ++k) {
        if (n_pix[k] <= 0 || n_obs[k] <= 0 || n_obs[k] > CCDGPU_MAX_OBS)
            return enc_fail(k, " has no pixels / observations");
        if (off[k] < 0 || off[k] + CCD_ENC_HDR > off[k + 1] || pixo[k] != pb)
            return fail(CCDGPU_EINVAL, "encoded batch: bad chip table entry " + std::to_string(k));
        const uint8_t *sec = enc + off[k];
        const ccd_enc_hdr *h = reinterpret_cast<const ccd_enc_hdr *>(sec);
        if ((h->mode != CCD_ENC_MODE_RAW && h->mode != CCD_ENC_MODE_COLS && h->mode != CCD_ENC_MODE_PACK) ||
            h->n_pix != n_pix[k] || h->n_obs != n_obs[k] || h->data_off != db ||
            (h->mode != CCD_ENC_MODE_RAW && (h->n_pal < 1 || h->n_pal > 16)))
            return enc_fail(k, " header does not match its shape");
        // the section holds everything its mode's layout addresses (the decoder trusts it)
        const int64_t np_ = n_pix[k], plane = np_ * n_obs[k], sec_bytes = off[k + 1] - off[k];
        const int32_t no_ = n_obs[k];
        const uint32_t *koff = reinterpret_cast<const uint32_t *>(ccd_enc_koff(sec));
        int rc;
        if (h->mode == CCD_ENC_MODE_RAW) {
            if (sec_bytes < ccd_enc_size_raw(plane)) return enc_fail(k, " raw section is truncated");
        } else if (h->mode == CCD_ENC_MODE_PACK) {
            // bit-packed runs: the kept table as in mode 1, then every run's descriptor against the
            // prefix sums of its code words (ceil(k w / 32)) and exceptions, the totals against the
            // header, and the section long enough for all five parts and the pad word -- after
            // this no code bit can send the decoder outside the section
            *packed = true;
            const int64_t kept = h->kept, code_words = h->code_words, exc_total = h->exc_total;
            if (kept < 0 || kept > plane || h->band_stride != 0 || code_words < 0 || exc_total < 0 ||
                code_words > 4 * plane + 8 * np_ || exc_total > 7 * plane ||
                sec_bytes < ccd_enc_size_pack_fixed(np_, no_))
                return enc_fail(k, " packed header does not fit its section");
            if ((rc = enc_check_koff(k, koff, np_, no_, kept))) return rc;
            const ccd_enc_run *runs = reinterpret_cast<const ccd_enc_run *>(ccd_enc_body(sec, np_, no_));
            int64_t cw = 0, ex = 0;
            for (int64_t r = 0; r < CCD_ENC_BANDS * np_; ++r) {
                const ccd_enc_run &d = runs[r];
                const int64_t kk = (int64_t)(koff[r / CCD_ENC_BANDS + 1] - koff[r / CCD_ENC_BANDS]);
                if (d.w > 16) return enc_fail(k, " run " + std::to_string(r) + " has a width above 16");
                if ((int64_t)d.code_word != cw || (int64_t)d.exc_off != ex)
                    return enc_fail(k, " run " + std::to_string(r) + " does not start at the prefix sums");
                if ((int64_t)d.n_exc > kk)
                    return enc_fail(k, " run " + std::to_string(r) + " has more exceptions than values");
                cw += (kk * d.w + 31) / 32;
                ex += d.n_exc;
            }
            if (cw != code_words || ex != exc_total)
                return enc_fail(k, " run totals do not match code_words / exc_total");
            if (sec_bytes < ccd_enc_size_pack(np_, no_, code_words, exc_total))
                return enc_fail(k, " packed section is truncated");
        } else {
            mode1 = true;
            const int64_t kept = h->kept, bstride = h->band_stride;
            if (kept < 0 || kept > plane || bstride < kept || bstride % 8 != 0 ||
                sec_bytes < ccd_enc_size_cols(np_, no_, bstride))
                return enc_fail(k, " band columns do not fit its section");
            if ((rc = enc_check_koff(k, koff, np_, no_, kept))) return rc;
        }
        pb += n_pix[k];
        db += (int64_t)n_pix[k] * n_obs[k];
    }
    if (pixo[n_chips] != pb) return fail(CCDGPU_EINVAL, "encoded batch: pixel total does not match");
    if (mode1 && *packed) return fail(CCDGPU_EINVAL, "encoded batch: mode 1 and mode 2 sections in one batch");
    return 0;
}

int ccdgpu_encoded_check(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs, const uint8_t *enc,
                         int64_t enc_bytes) {
    bool packed;
    return encoded_check(n_chips, n_pix, n_obs, enc, enc_bytes, &packed);
}

int ccdgpu_stage_slot_encoded(ccdgpu_ctx *c, int32_t slot, const ccdgpu_params *params, int32_t n_chips,
                              const int32_t *n_pix, const int32_t *n_obs, const int64_t *dates, const uint8_t *enc,
                              int64_t enc_bytes) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (slot < 0 || slot >= CCDGPU_UPLOAD_SLOTS)
        return fail(CCDGPU_EINVAL, "slot must be in 0 .. " + std::to_string(CCDGPU_UPLOAD_SLOTS - 1));
    if (c->pending && slot == c->pend_slot)
        return fail(CCDGPU_EINVAL, "slot " + std::to_string(slot) + " is read by the detection begun with ccdgpu_run_slot_begin");
    if (!dates || !enc) return fail(CCDGPU_EINVAL, "NULL input buffer");
    Shape sh;
    int rc = make_shape(n_chips, n_pix, n_obs, sh);
    if (rc || (rc = check_params(params))) return rc;
    bool packed = false;
    if ((rc = encoded_check(n_chips, n_pix, n_obs, enc, enc_bytes, &packed))) return rc;
    // a batch with bit-packed sections is always decoded into the slot's standard buffers (the
    // detection kernel reads modes 0 and 1 in place, not mode 2)
    const bool decode = c->decode_enc || packed;
    const int64_t *off = ccd_enc_chip_off(enc);
    const int64_t pb = sh.total_pix();
    HIPCHK(hipSetDevice(c->device));
    const size_t tobs = (size_t)sh.total_obs(), tdata = (size_t)sh.total_data();
    if ((rc = c->slot_dates[slot].ensure(tobs)) || (rc = c->slot_enc[slot].ensure((size_t)off[n_chips])))
        return rc;
    if (decode && ((rc = c->slot_spectra[slot].ensure(7 * tdata)) || (rc = c->slot_qa[slot].ensure(tdata))))
        return rc;
    // upload on the copy stream; the detection kernel reads the encoded batch in place (no decode
    // pass: px_setup in ccd_kernels.hip), or -- CCDGPU_DECODE=1 -- it is decoded there into the
    // slot's standard buffers first.  run_slot waits for the copy stream through the slot's event.
    HIPCHK(hipMemcpyAsync(c->slot_dates[slot].p, dates, sizeof(int64_t) * tobs, hipMemcpyHostToDevice, c->up_stream));
    HIPCHK(hipMemcpyAsync(c->slot_enc[slot].p, enc, (size_t)off[n_chips], hipMemcpyHostToDevice, c->up_stream));
    HIPCHK(hipEventRecord(c->uploaded[slot], c->up_stream));
    if (decode) {
        if (c->up_stream != c->copy_stream) HIPCHK(hipStreamWaitEvent(c->copy_stream, c->uploaded[slot], 0));
        if (packed) {
            if (ccdk_decode_pack(c->slot_enc[slot].p, pb, c->slot_spectra[slot].p, c->slot_qa[slot].p, c->copy_stream))
                return fail(CCDGPU_EHIP, "ccd_decode_pack launch failed");
        } else if (ccdk_decode_enc(c->slot_enc[slot].p, pb, c->slot_spectra[slot].p, c->slot_qa[slot].p, c->copy_stream))
            return fail(CCDGPU_EHIP, "ccd_decode_enc launch failed");
        HIPCHK(hipEventRecord(c->uploaded[slot], c->copy_stream));
    }
    c->slot_shape[slot] = sh;
    c->slot_params[slot] = *params;
    c->slot_ready[slot] = true;
    c->slot_encoded[slot] = !decode;
    return 0;
}

int ccdgpu_stage_slot(ccdgpu_ctx *c, int32_t slot, const ccdgpu_params *params, int32_t n_chips, int32_t n_pix,
                      int32_t n_obs, const int64_t *dates, const int16_t *spectra, const uint16_t *qa) {
    std::vector<int32_t> np, no;
    uniform(n_chips, n_pix, n_obs, np, no);
    return ccdgpu_stage_slot_chips(c, slot, params, n_chips, np.data(), no.data(), dates, spectra, qa);
}

static int slot_inputs(ccdgpu_ctx *c, int32_t slot) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (c->pending) return fail(CCDGPU_EINVAL, "a detection begun with ccdgpu_run_slot_begin is not finished");
    if (slot < 0 || slot >= CCDGPU_UPLOAD_SLOTS || !c->slot_ready[slot]) return fail(CCDGPU_EINVAL, "slot has no staged batch");
    int rc = stage_alloc(c, &c->slot_params[slot], c->slot_shape[slot], nullptr, false);
    if (rc) return rc;
    HIPCHK(hipStreamWaitEvent(c->aux, c->uploaded[slot], 0));
    c->in_dates = c->slot_dates[slot].p;
    c->in_enc = c->slot_encoded[slot] ? c->slot_enc[slot].p : nullptr;
    c->in_spectra = c->slot_encoded[slot] ? nullptr : c->slot_spectra[slot].p;
    c->in_qa = c->slot_encoded[slot] ? nullptr : c->slot_qa[slot].p;
    c->staged = true;
    c->ran = false;
    if (!c->keep_slots) c->slot_ready[slot] = false;
    return 0;
}

int ccdgpu_run_slot(ccdgpu_ctx *c, int32_t slot, double *kernel_seconds) {
    int rc = slot_inputs(c, slot);
    return rc ? rc : ccdgpu_run_staged(c, kernel_seconds);
}

static void detect_args(ccdgpu_ctx *c, CcdDetectArgs &a);
static int launch(ccdgpu_ctx *c, CcdDetectArgs &a);
static int finish(ccdgpu_ctx *c, double *kernel_seconds, bool *again, bool chained = false);

int ccdgpu_run_slot_begin(ccdgpu_ctx *c, int32_t slot) {
    int rc = slot_inputs(c, slot);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    detect_args(c, c->pend_args);
    if ((rc = launch(c, c->pend_args))) return rc;
    c->pending = true;
    c->pend_slot = slot;
    return 0;
}

int ccdgpu_run_query(ccdgpu_ctx *c) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (!c->pending) return 1;
    const hipError_t e = hipEventQuery(c->rows_mode ? c->done_rows : c->done);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) return 0;
    return fail(CCDGPU_EHIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
}

int ccdgpu_run_slot_end(ccdgpu_ctx *c, double *kernel_seconds) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (!c->pending) return fail(CCDGPU_EINVAL, "no detection begun with ccdgpu_run_slot_begin");
    if (c->rows_mode) return fail(CCDGPU_EINVAL, "a detection begun with ccdgpu_run_slot_begin_rows ends with ccdgpu_run_slot_end_rows");
    HIPCHK(hipSetDevice(c->device));
    c->pending = false;
    c->pend_slot = -1;
    for (int attempt = 0; attempt < 4; ++attempt) {
        bool again = false;
        const int rc = finish(c, kernel_seconds, &again);
        if (!again) return rc;
        if (int rc2 = launch(c, c->pend_args)) return rc2;
    }
    return fail(CCDGPU_EOVERFLOW, "segment pool kept overflowing");
}

// An error after a detection was queued (the chain behind it could not be enqueued): wait for
// everything the context queued, so no kernel still reads the slot or writes the pool when the
// caller recovers and restages, then return the error.
static int drain_after_error(ccdgpu_ctx *c, int rc) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->aux);
    c->pending = false;
    c->rows_mode = false;
    c->pend_slot = -1;
    return rc;
}

// The rest of a batch behind its detection, all on the aux stream (which already waits for the
// detection's end): CSR offsets (scan), the closing entry and rows per pixel, row offsets
// (scan), pool -> CSR with the device's segment count, row packing per chip, then the copies of
// the CSR offsets (pinned staging), row offsets, rows (up to the caller's capacity) and mask
// words into the caller's buffers.  Capacities are sized for any segment count the pool holds.
static int enqueue_rows(ccdgpu_ctx *c) {
    const Shape &sh = c->shape;
    const int nc = sh.n_chips();
    const int64_t np = c->total_pix;
    hipStream_t ax = c->aux;
    int rc;
    const int64_t rows_dev = np + c->pool_cap;  // rows <= pixels + segments
    if ((rc = c->csr.ensure(c->pool_cap > 0 ? c->pool_cap : 1)) || (rc = c->rows.ensure((size_t)rows_dev)) ||
        (rc = c->row_off.ensure(np + 1)) || (rc = c->rowcnt.ensure(np + 1)) || (rc = c->offsets.ensure(np + 1)) ||
        (rc = c->h_off.ensure(sizeof(int64_t) * (size_t)(np + 1))))
        return rc;
    // temporary storage of both scans (their instantiations differ: int32 counts -> int64 offsets,
    // int64 row counts -> int64 row offsets), each called with its own size
    size_t tmp_seg = 0, tmp_row = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_seg, c->nseg.p, c->offsets.p, (int)np, ax));
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_row, c->rowcnt.p, c->row_off.p, (int)np + 1, ax));
    if ((rc = c->cub_tmp.ensure(std::max(tmp_seg, tmp_row)))) return rc;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(c->cub_tmp.p, tmp_seg, c->nseg.p, c->offsets.p, (int)np, ax));
    if (ccdk_row_counts(c->nseg.p, c->offsets.p, np, c->rowcnt.p, ax)) return fail(CCDGPU_EHIP, "row count launch failed");
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(c->cub_tmp.p, tmp_row, c->rowcnt.p, c->row_off.p, (int)np + 1, ax));
    // (on a pool overflow -- counters[3] -- the segment counts exceed what the pool holds: the scatter
    // and the row packing write nothing and ccdgpu_run_slot_end_rows reruns the batch)
    // the chips' (cx, cy) through pinned staging
    if ((rc = c->row_xy.ensure(2 * (size_t)nc)) || (rc = c->h_xy.ensure(sizeof(int32_t) * 2 * (size_t)nc))) return rc;
    int32_t *hxy = reinterpret_cast<int32_t *>(c->h_xy.p);
    for (int32_t ch = 0; ch < nc; ++ch) {
        hxy[2 * ch] = c->rq_cx[ch];
        hxy[2 * ch + 1] = c->rq_cy[ch];
    }
    HIPCHK(hipMemcpyAsync(c->row_xy.p, hxy, sizeof(int32_t) * 2 * (size_t)nc, hipMemcpyHostToDevice, ax));
    if (c->rows_fused) {
        // pool -> CSR and rows in one pass, then the default rows of pixels without a model
        if (ccdk_pool_rows(c->pool.p, c->pool_seq.p, c->counters.p + 1, 0, c->counters.p + 3, c->pool_cap, c->offsets.p,
                           c->chip_pix_off.p, nc, c->csr.p, c->row_off.p, c->row_xy.p,
                           c->rq_width, c->rows.p, rows_dev, 256, ax) ||
            ccdk_default_rows(c->nseg.p, np, c->counters.p + 3, c->chip_pix_off.p, nc, c->row_off.p, c->row_xy.p, c->rq_width,
                              c->rows.p, rows_dev, ax))
            return fail(CCDGPU_EHIP, "row packing launch failed");
    } else {
        if (ccdk_scatter_dev(c->pool.p, c->pool_seq.p, c->counters.p + 1, c->counters.p + 3, c->pool_cap, c->offsets.p,
                             c->chip_pix_off.p, nc, c->csr.p, ax))
            return fail(CCDGPU_EHIP, "scatter launch failed");
        for (int32_t ch = 0; ch < nc; ++ch) {
            const int64_t q = sh.pix_off[ch];
            if (ccdk_pack_rows(c->csr.p, c->offsets.p + q, c->row_off.p + q, c->mask.p + (size_t)q * c->mask_words,
                               c->mask_words, sh.npix[ch], sh.nobs[ch], c->rq_cx[ch], c->rq_cy[ch], c->rq_width, c->rows.p,
                               nullptr, c->counters.p + 3, c->pool_cap, rows_dev, ax))
                return fail(CCDGPU_EHIP, "row packing launch failed");
        }
    }
    const size_t ob = sizeof(int64_t) * (size_t)(np + 1);
    HIPCHK(hipMemcpyAsync(c->h_off.p, c->offsets.p, ob, hipMemcpyDeviceToHost, ax));
    HIPCHK(hipMemcpyAsync(c->rq_offsets, c->row_off.p, ob, hipMemcpyDeviceToHost, ax));
    const int64_t nrc = std::min<int64_t>(c->rq_rows_cap, rows_dev);
    if (nrc > 0) HIPCHK(hipMemcpyAsync(c->rq_rows, c->rows.p, sizeof(ccdgpu_row) * (size_t)nrc, hipMemcpyDeviceToHost, ax));
    const size_t nbits = (size_t)np * c->mask_words;
    if (nbits > 0) HIPCHK(hipMemcpyAsync(c->rq_mask, c->mask.p, sizeof(uint32_t) * nbits, hipMemcpyDeviceToHost, ax));
    HIPCHK(hipEventRecord(c->done_rows, ax));
    return 0;
}

int ccdgpu_run_slot_begin_rows(ccdgpu_ctx *c, int32_t slot, const int32_t *cx, const int32_t *cy, int32_t width,
                               int64_t *row_offsets, int64_t offsets_cap, ccdgpu_row *rows, int64_t rows_cap,
                               uint32_t *mask_bits, int64_t mask_cap) {
    if (!c || !cx || !cy || !row_offsets || !rows || !mask_bits) return fail(CCDGPU_EINVAL, "NULL argument");
    if (width <= 0) return fail(CCDGPU_EINVAL, "width must be > 0");
    if (c->pending) return fail(CCDGPU_EINVAL, "a detection begun with ccdgpu_run_slot_begin is not finished");
    if (slot < 0 || slot >= CCDGPU_UPLOAD_SLOTS || !c->slot_ready[slot]) return fail(CCDGPU_EINVAL, "slot has no staged batch");
    const Shape &ssh = c->slot_shape[slot];
    const int64_t np = ssh.total_pix();
    const int64_t words = (ssh.n_obs_max + 31) / 32;
    if (offsets_cap < np + 1 || mask_cap < np * words)
        return fail(CCDGPU_EINVAL, "run_slot_begin_rows: offsets / mask buffers too small (need " + std::to_string(np + 1) +
                                       " offsets, " + std::to_string(np * words) + " mask words)");
    int rc = slot_inputs(c, slot);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    c->rq_offsets = row_offsets;
    c->rq_offsets_cap = offsets_cap;
    c->rq_rows = rows;
    c->rq_rows_cap = rows_cap;
    c->rq_mask = mask_bits;
    c->rq_mask_cap = mask_cap;
    c->rq_width = width;
    const int nc = c->shape.n_chips();
    c->rq_cx.assign(cx, cx + nc);
    c->rq_cy.assign(cy, cy + nc);
    detect_args(c, c->pend_args);
    if ((rc = launch(c, c->pend_args))) return rc;
    if ((rc = enqueue_rows(c))) return drain_after_error(c, rc);
    c->pending = true;
    c->rows_mode = true;
    c->pend_slot = slot;
    return 0;
}

int ccdgpu_run_slot_end_rows(ccdgpu_ctx *c, double *kernel_seconds, int64_t *n_rows) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (n_rows) *n_rows = 0;
    if (!c->pending || !c->rows_mode) return fail(CCDGPU_EINVAL, "no detection begun with ccdgpu_run_slot_begin_rows");
    HIPCHK(hipSetDevice(c->device));
    c->pending = false;
    c->rows_mode = false;
    c->pend_slot = -1;
    int rc = 0;
    for (int attempt = 0;; ++attempt) {
        HIPCHK(hipEventSynchronize(c->done_rows));
        bool again = false;
        rc = finish(c, kernel_seconds, &again, true);
        if (!again) break;
        if (attempt == 3) return fail(CCDGPU_EOVERFLOW, "segment pool kept overflowing");
        int rc2;
        if ((rc2 = launch(c, c->pend_args))) return rc2;
        if ((rc2 = enqueue_rows(c))) return drain_after_error(c, rc2);
    }
    if (rc && rc != CCDGPU_EQA) return rc;
    const int64_t nr = c->rq_offsets[c->total_pix];
    if (n_rows) *n_rows = nr;
    if (nr > c->rq_rows_cap) {
        // the run is complete (ccdgpu_fetch_batch_rows_into fetches it into larger buffers); an
        // unsupported QA value outranks the short buffer -- CCDGPU_EQA with *n_rows set, so the
        // caller both fetches every row and raises pyccd's ValueError
        if (rc == CCDGPU_EQA) return rc;
        return fail(CCDGPU_EOVERFLOW, "run_slot_end_rows: " + std::to_string(nr) + " rows, the buffer holds " +
                                          std::to_string(c->rq_rows_cap));
    }
    return rc;
}

int ccdgpu_staged_inputs(ccdgpu_ctx *c, int16_t *spectra, uint16_t *qa) {
    if (!c || !c->staged) return fail(CCDGPU_EINVAL, "nothing staged");
    HIPCHK(hipSetDevice(c->device));
    const size_t tdata = (size_t)c->shape.total_data();
    const int16_t *ins = c->in_spectra;
    const uint16_t *inq = c->in_qa;
    if (c->in_enc) {
        // an encoded batch read in place by the detection: decoded here (the standalone decoder,
        // the same mapping as px_setup's) into the context's standard buffers
        int rc;
        if ((rc = c->spectra.ensure(7 * tdata)) || (rc = c->qa.ensure(tdata))) return rc;
        if (ccdk_decode_enc(c->in_enc, c->shape.total_pix(), c->spectra.p, c->qa.p, c->stream))
            return fail(CCDGPU_EHIP, "ccd_decode_enc launch failed");
        ins = c->spectra.p;
        inq = c->qa.p;
    }
    if (spectra)
        HIPCHK(hipMemcpyAsync(spectra, ins, sizeof(int16_t) * 7 * tdata, hipMemcpyDeviceToHost, c->stream));
    if (qa) HIPCHK(hipMemcpyAsync(qa, inq, sizeof(uint16_t) * tdata, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

static void detect_args(ccdgpu_ctx *c, CcdDetectArgs &a) {
    const ccdgpu_params &p = c->params;
    const Shape &sh = c->shape;
    const int nc = sh.n_chips();
    std::memset(&a, 0, sizeof(a));
    a.p = p;
    a.n_chips = nc;
    a.n_obs_max = sh.n_obs_max;
    a.mask_words = c->mask_words;
    a.n_slots = c->n_slots;
    a.poison = c->poison;
    a.total_pix = c->total_pix;
    a.chip_nobs = c->chip_nobs.p;
    a.chip_obs_off = c->chip_obs_off.p;
    a.chip_pix_off = c->chip_pix_off.p;
    a.chip_data_off = c->chip_data_off.p;
    a.spectra = c->in_spectra;
    a.qa = c->in_qa;
    a.enc = c->in_enc;
    a.order = c->order.p;
    a.sdates = c->sdates.p;
    a.basis = c->basis.p;
    a.counters = c->counters.p;
    a.s_date = c->s_date.p;
    a.s_row = c->s_row.p;
    a.s_bk = c->s_bk.p;
    a.s_f64 = c->s_f64.p;
    a.mask_bits = c->mask.p;
    a.procedure = c->procedure.p;
    a.probs = c->probs.p;
    a.nseg = c->nseg.p;
    a.stats = c->stats.p;
    for (int k = 0; k <= CCDGPU_MAX_PEEK; ++k) {
        if (k <= p.peek_size) a.thr_table[k] = p.change_threshold;
        else a.thr_table[k] = chi2_5_ppf(1.0 - std::pow(1.0 - p.change_probability, (double)p.peek_size / k));
    }
}

static int launch(ccdgpu_ctx *c, CcdDetectArgs &a) {
    const ccdgpu_params &p = c->params;
    const Shape &sh = c->shape;
    const int nc = sh.n_chips();
    a.pool = c->pool.p;
    a.pool_seq = c->pool_seq.p;
    a.pool_cap = c->pool_cap;
    // h_small: [0, 64) initial counters, [64, 128) counters back, [128, 128 + 8 NSTATS) stats
    // back, then the kernel arguments (each launch waits for the previous one's copies)
    // [SM_ARGS + args, + 8 NSTATS) zeros for the statistics
    constexpr size_t SM_ARGS = 128 + 8 * CCD_NSTATS;
    constexpr size_t SM_ZERO = SM_ARGS + ((sizeof(CcdDetectArgs) + 63) & ~(size_t)63);
    if (int rc0 = c->h_small.ensure(SM_ZERO + 8 * CCD_NSTATS)) return rc0;
    unsigned long long *hinit = reinterpret_cast<unsigned long long *>(c->h_small.p);
    const unsigned long long init[8] = {0ull, 0ull, ~0ull, 0ull, 0ull, ~0ull, 0ull, ~0ull};
    std::memcpy(hinit, init, sizeof(init));
    std::memset(c->h_small.p + SM_ZERO, 0, 8 * CCD_NSTATS);
    hipStream_t ax = c->aux;
    HIPCHK(hipMemcpyAsync(c->counters.p, hinit, sizeof(init), hipMemcpyHostToDevice, ax));
    HIPCHK(hipMemcpyAsync(c->stats.p, c->h_small.p + SM_ZERO, 8 * CCD_NSTATS, hipMemcpyHostToDevice, ax));
    CcdDetectArgs *hargs = reinterpret_cast<CcdDetectArgs *>(c->h_small.p + SM_ARGS);
    std::memcpy(hargs, &a, sizeof(a));
    if (ccdk_set_args(hargs, c->arg_slot, ax)) return fail(CCDGPU_EHIP, "copying kernel arguments to constant memory failed");
    HIPCHK(hipEventRecord(c->ev[0], ax));
    if (ccdk_prep(c->in_dates, nc, c->chip_nobs.p, c->chip_obs_off.p, p.avg_days_yr, p.argsort_stable, c->order.p,
                  c->sdates.p, c->basis.p, ax))
        return fail(CCDGPU_EHIP, std::string("prep launch: ") + hipGetErrorString(hipGetLastError()));
    HIPCHK(hipEventRecord(c->ev[1], ax));
    if (ax != c->stream) HIPCHK(hipStreamWaitEvent(c->stream, c->ev[1], 0));
    if (ccdk_detect(c->n_slots, c->variant, sh.n_obs_max, c->arg_slot, c->stream))
        return fail(CCDGPU_EHIP, std::string("detect launch: ") + hipGetErrorString(hipGetLastError()));
    HIPCHK(hipEventRecord(c->ev[2], c->stream));
    if (ax != c->stream) HIPCHK(hipStreamWaitEvent(ax, c->ev[2], 0));
    // counters and statistics back into pinned memory; `done` marks their arrival (finish sleeps on it)
    unsigned long long *h = reinterpret_cast<unsigned long long *>(c->h_small.p + 64);
    unsigned long long *hst = reinterpret_cast<unsigned long long *>(c->h_small.p + 128);
    HIPCHK(hipMemcpyAsync(h, c->counters.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ax));
    HIPCHK(hipMemcpyAsync(hst, c->stats.p, sizeof(unsigned long long) * CCD_NSTATS, hipMemcpyDeviceToHost, ax));
    if (c->done) HIPCHK(hipEventRecord(c->done, ax));
    return 0;
}

static int finish(ccdgpu_ctx *c, double *kernel_seconds, bool *again, bool chained) {
    const ccdgpu_params &p = c->params;
    const Shape &sh = c->shape;
    const int nc = sh.n_chips();
    hipStream_t ax = c->aux;
    unsigned long long *h = reinterpret_cast<unsigned long long *>(c->h_small.p + 64);
    unsigned long long *hst = reinterpret_cast<unsigned long long *>(c->h_small.p + 128);
    *again = false;
    if (chained) {
        // the batch chain has completed (the caller waited for done_rows)
    } else if (c->done) {
        HIPCHK(hipEventSynchronize(c->done));
    } else {
        HIPCHK(hipStreamSynchronize(ax));
    }
    if (h[4] >= 100000) {
        // checking build: every call site that ran without a full EXEC, from the line bitmap
        // (bit = line / 2) in stats[8 ..]
        const unsigned long long *st = hst;
        std::string lines;
        for (int w = 8; w < CCD_NSTATS; ++w)
            for (int b = 0; b < 64; ++b)
                if ((st[w] >> b) & 1ull) {
                    const int l0 = 2 * (64 * (w - 8) + b);
                    lines += (lines.empty() ? "" : ", ") + std::to_string(l0) + "-" + std::to_string(l0 + 1);
                }
        return fail(CCDGPU_EHIP, "cross-lane primitive ran without a full EXEC at ccd_kernels.hip line " +
                                     std::to_string(h[4] - 100000) + " (all call sites: lines " + lines + ")");
    }
    if (h[4]) return fail(CCDGPU_EHIP, "kernel index guard tripped at ccd_kernels.hip line " + std::to_string(h[4]));
    if (h[3]) {  // pool overflow: grow and rerun
        c->pool_cap = (int64_t)(h[1] + h[1] / 4 + 1024);
        ++c->pool_reruns;
        int rc;
        if ((rc = c->pool.ensure(c->pool_cap)) || (rc = c->pool_seq.ensure(c->pool_cap))) return rc;
        *again = true;
        return 0;
    }
    c->n_pool = (int64_t)h[1];
    float ms_prep = 0.f, ms_det = 0.f;
    (void)hipEventElapsedTime(&ms_prep, c->ev[0], c->ev[1]);
    (void)hipEventElapsedTime(&ms_det, c->ev[1], c->ev[2]);
    const unsigned long long *st = hst;
    for (int i = 0; i < CCD_NSTATS; ++i) c->diag[i] = st[i];
    int rc;
    if (chained) {
        // CSR, offsets and rows were made by the chain (enqueue_rows); the offsets are in h_off
        c->h_offsets.resize(c->total_pix + 1);
        std::memcpy(c->h_offsets.data(), c->h_off.p, sizeof(int64_t) * (size_t)(c->total_pix + 1));
    } else {
    // CSR: exclusive scan of per-pixel counts, then scatter the pool
    if ((rc = c->csr.ensure(c->n_pool > 0 ? c->n_pool : 1))) return rc;
    size_t tmp_bytes = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, c->nseg.p, c->offsets.p, (int)c->total_pix + 1, ax));
    if ((rc = c->cub_tmp.ensure(tmp_bytes))) return rc;
    // nseg has total_pix entries; the scan over total_pix+1 needs a trailing zero
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(c->cub_tmp.p, tmp_bytes, c->nseg.p, c->offsets.p, (int)c->total_pix, ax));
    c->h_offsets.resize(c->total_pix + 1);
    if ((rc = c->h_off.ensure(sizeof(int64_t) * (size_t)c->total_pix))) return rc;
    HIPCHK(hipMemcpyAsync(c->h_off.p, c->offsets.p, sizeof(int64_t) * c->total_pix, hipMemcpyDeviceToHost, ax));
    HIPCHK(hipStreamSynchronize(ax));
    std::memcpy(c->h_offsets.data(), c->h_off.p, sizeof(int64_t) * (size_t)c->total_pix);
    c->h_offsets[c->total_pix] = c->n_pool;
    if (c->rows_fused ? ccdk_pool_rows(c->pool.p, c->pool_seq.p, nullptr, c->n_pool, nullptr, c->n_pool, c->offsets.p,
                                       c->chip_pix_off.p, nc, c->csr.p, nullptr, nullptr, 1, nullptr, 0, 256, ax)
                      : ccdk_scatter(c->pool.p, c->pool_seq.p, c->n_pool, c->offsets.p, c->chip_pix_off.p, nc, c->csr.p, ax))
        return fail(CCDGPU_EHIP, "scatter launch failed");
    HIPCHK(hipEventRecord(c->ev[3], ax));
    HIPCHK(hipStreamSynchronize(ax));
    }
    c->last.detect_ms = ms_det;
    c->last.detect_ms_device = h[6] > h[5] ? (double)(h[6] - h[5]) / 1e5 : 0.0;  // 100 MHz clock
    c->last.prep_ms = ms_prep;
    c->last.pixels = c->total_pix;
    c->last.segments = c->n_pool;
    c->last.lasso_fits = (int64_t)st[0];
    c->last.cd_sweeps = (int64_t)st[1];
    c->last.flops = (int64_t)st[2];
    c->last.pool_reruns = c->pool_reruns;
    c->last.pool_cap = c->pool_cap;
    c->last.wave_slots = c->n_slots;
    c->last.n_cu = c->n_cu;
    const int64_t in_bytes = sh.total_data() * 16 + sh.total_obs() * 8;
    const int64_t out_bytes = c->n_pool * (int64_t)sizeof(ccdgpu_segment) + c->total_pix * ((int64_t)c->mask_words * 4 + 4 + 24 + 4);
    c->last.bytes = in_bytes + out_bytes;
    if (kernel_seconds) *kernel_seconds = (ms_prep + ms_det) * 1e-3;
    c->ran = true;
    if (h[7] != ~0ull)
        return fail(CCDGPU_EOVERFLOW, "adaptive peek of pixel " + std::to_string(h[7]) + " exceeds " +
                                          std::to_string(CCDGPU_MAX_PEEK) + " observations (PEEK_SIZE " +
                                          std::to_string(p.peek_size) + ")");
    if (h[2] != ~0ull) {
        g_err = "unsupported bit-packed QA value (pixel " + std::to_string(h[2]) + ")";
        return CCDGPU_EQA;
    }
    return 0;
}

int ccdgpu_run_staged(ccdgpu_ctx *c, double *kernel_seconds) {
    if (!c || !c->staged) return fail(CCDGPU_EINVAL, "nothing staged");
    if (c->pending) return fail(CCDGPU_EINVAL, "a detection begun with ccdgpu_run_slot_begin is not finished");
    HIPCHK(hipSetDevice(c->device));
    CcdDetectArgs a;
    detect_args(c, a);
    for (int attempt = 0; attempt < 4; ++attempt) {
        int rc = launch(c, a);
        if (rc) return rc;
        bool again = false;
        rc = finish(c, kernel_seconds, &again);
        if (!again) return rc;
    }
    return fail(CCDGPU_EOVERFLOW, "segment pool kept overflowing");
}

int ccdgpu_diag_counters(ccdgpu_ctx *c, uint64_t *out, int32_t n) {
    if (!c || !out || n < 0) return fail(CCDGPU_EINVAL, "bad argument");
    for (int i = 0; i < n && i < CCD_NSTATS; ++i) out[i] = c->diag[i];
    return 0;
}

int ccdgpu_last_stats(ccdgpu_ctx *c, ccdgpu_stats *s) {
    if (!c || !s) return fail(CCDGPU_EINVAL, "NULL argument");
    *s = c->last;
    return 0;
}

static int fetch_chip(ccdgpu_ctx *c, int32_t chip, ccdgpu_result *out) {
    std::memset(out, 0, sizeof(*out));
    if (!c->ran) return fail(CCDGPU_EINVAL, "no completed run to fetch");
    if (chip < 0 || chip >= c->shape.n_chips()) return fail(CCDGPU_EINVAL, "chip index out of range");
    HIPCHK(hipSetDevice(c->device));
    const int np = c->shape.npix[chip], no = c->shape.nobs[chip];
    const int64_t p0 = c->shape.pix_off[chip], o0 = c->shape.obs_off[chip];
    const int64_t s0 = c->h_offsets[p0], s1 = c->h_offsets[p0 + np];
    out->n_pix = np;
    out->n_obs = no;
    out->n_seg = s1 - s0;
    out->mask_words = c->mask_words;
    out->error_pixel = -1;
    out->seg_offsets = (int64_t *)std::malloc(sizeof(int64_t) * (np + 1));
    out->segments = (ccdgpu_segment *)std::malloc(sizeof(ccdgpu_segment) * (size_t)(out->n_seg + 1));
    out->mask_bits = (uint32_t *)std::malloc(sizeof(uint32_t) * (size_t)np * c->mask_words + 4);
    out->procedure = (int32_t *)std::malloc(sizeof(int32_t) * np);
    out->probs = (double *)std::malloc(sizeof(double) * 3 * np);
    out->sorted_dates = (int64_t *)std::malloc(sizeof(int64_t) * no);
    out->sort_index = (int32_t *)std::malloc(sizeof(int32_t) * no);
    if (!out->seg_offsets || !out->segments || !out->mask_bits || !out->procedure || !out->probs ||
        !out->sorted_dates || !out->sort_index) {
        ccdgpu_result_free(out);
        return fail(CCDGPU_ENOMEM, "host allocation failed");
    }
    for (int i = 0; i <= np; ++i) out->seg_offsets[i] = c->h_offsets[p0 + i] - s0;
    if (out->n_seg > 0)
        HIPCHK(hipMemcpyAsync(out->segments, c->csr.p + s0, sizeof(ccdgpu_segment) * out->n_seg, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out->mask_bits, c->mask.p + (size_t)p0 * c->mask_words, sizeof(uint32_t) * (size_t)np * c->mask_words, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out->procedure, c->procedure.p + p0, sizeof(int32_t) * np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out->probs, c->probs.p + 3 * p0, sizeof(double) * 3 * np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out->sorted_dates, c->sdates.p + o0, sizeof(int64_t) * no, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out->sort_index, c->order.p + o0, sizeof(int32_t) * no, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < np; ++i)
        if (out->procedure[i] < 0) {
            out->error_pixel = i;
            break;
        }
    return 0;
}

// Rows of chips [c0, c1) of the last run, packed on the device and copied back in one piece:
// row offsets over the chips' pixels, rows pixel-major, and the masks either one byte per date
// (packed_mask false: chip c's block at data_off[c] - data_off[c0], [n_pix_c][n_obs_c]) or as the
// device's bit words ([pixels][mask_words]).
static int fetch_rows_range(ccdgpu_ctx *c, int32_t c0, int32_t c1, const int32_t *cx, const int32_t *cy, int32_t width,
                            ccdgpu_rows *out, bool packed_mask) {
    std::memset(out, 0, sizeof(*out));
    if (!c->ran) return fail(CCDGPU_EINVAL, "no completed run to fetch");
    if (width <= 0) return fail(CCDGPU_EINVAL, "width must be > 0");
    HIPCHK(hipSetDevice(c->device));
    const Shape &sh = c->shape;
    const int64_t p0 = sh.pix_off[c0], np = sh.pix_off[c1] - p0;
    const int64_t d0 = sh.data_off[c0], nd = sh.data_off[c1] - d0;
    const int64_t s0 = c->h_offsets[p0];
    // rows per pixel = max(1, segments): host prefix over the segment offsets already here
    std::vector<int64_t> soff((size_t)np + 1), roff((size_t)np + 1);
    roff[0] = 0;
    for (int64_t i = 0; i <= np; ++i) soff[i] = c->h_offsets[p0 + i] - s0;
    for (int64_t i = 0; i < np; ++i) roff[i + 1] = roff[i] + std::max<int64_t>(1, soff[i + 1] - soff[i]);
    const int64_t n_rows = roff[np];
    int rc;
    if ((rc = c->rows.ensure((size_t)n_rows)) || (rc = c->row_off.ensure(np + 1)) || (rc = c->seg_off1.ensure(np + 1)) ||
        (!packed_mask && (rc = c->mask8.ensure((size_t)nd))))
        return rc;
    // offsets through pinned staging, row packing and the copies back on the aux stream (the
    // reserved CUs when there are: other contexts' detections hold the rest)
    hipStream_t ax = c->aux;
    const size_t ob = sizeof(int64_t) * (size_t)(np + 1);
    if ((rc = c->h_fo.ensure(2 * ob))) return rc;
    std::memcpy(c->h_fo.p, soff.data(), ob);
    std::memcpy(c->h_fo.p + ob, roff.data(), ob);
    HIPCHK(hipMemcpyAsync(c->seg_off1.p, c->h_fo.p, ob, hipMemcpyHostToDevice, ax));
    HIPCHK(hipMemcpyAsync(c->row_off.p, c->h_fo.p + ob, ob, hipMemcpyHostToDevice, ax));
    for (int32_t ch = c0; ch < c1; ++ch) {
        const int64_t q = sh.pix_off[ch] - p0;
        if (ccdk_pack_rows(c->csr.p + s0, c->seg_off1.p + q, c->row_off.p + q, c->mask.p + (size_t)sh.pix_off[ch] * c->mask_words,
                           c->mask_words, sh.npix[ch], sh.nobs[ch], cx[ch - c0], cy[ch - c0], width, c->rows.p,
                           packed_mask ? nullptr : c->mask8.p + (sh.data_off[ch] - d0), nullptr, INT64_MAX, INT64_MAX, ax))
            return fail(CCDGPU_EHIP, "row packing launch failed");
    }
    out->n_pix = (int32_t)np;
    out->n_obs = c1 - c0 == 1 ? sh.nobs[c0] : 0;
    out->n_rows = n_rows;
    out->row_offsets = (int64_t *)std::malloc(sizeof(int64_t) * (np + 1));
    out->rows = (ccdgpu_row *)std::malloc(sizeof(ccdgpu_row) * (size_t)(n_rows > 0 ? n_rows : 1));
    const size_t nbits = (size_t)np * c->mask_words;
    if (packed_mask) {
        out->mask_words = c->mask_words;
        out->mask_bits = (uint32_t *)std::malloc(sizeof(uint32_t) * (nbits > 0 ? nbits : 1));
    } else {
        out->mask = (int8_t *)std::malloc((size_t)(nd > 0 ? nd : 1));
    }
    if (!out->row_offsets || !out->rows || (packed_mask ? !out->mask_bits : !out->mask)) {
        ccdgpu_rows_free(out);
        return fail(CCDGPU_ENOMEM, "host allocation failed");
    }
    std::memcpy(out->row_offsets, roff.data(), sizeof(int64_t) * (np + 1));
    const size_t row_bytes = sizeof(ccdgpu_row) * (size_t)n_rows;
    if (packed_mask) {
        // batch fetch: rows and mask words land in the context's pinned buffer by DMA (one copy
        // each at link speed), then go to the caller's buffers with a host memcpy
        const size_t bit_bytes = sizeof(uint32_t) * nbits;
        const size_t bit_at = (row_bytes + 255) & ~(size_t)255;
        if ((rc = c->h_rows.ensure(bit_at + bit_bytes))) {
            (void)hipStreamSynchronize(ax);
            ccdgpu_rows_free(out);
            return rc;
        }
        HIPCHK(hipMemcpyAsync(c->h_rows.p, c->rows.p, row_bytes, hipMemcpyDeviceToHost, ax));
        HIPCHK(hipMemcpyAsync(c->h_rows.p + bit_at, c->mask.p + (size_t)p0 * c->mask_words, bit_bytes,
                              hipMemcpyDeviceToHost, ax));
        HIPCHK(hipStreamSynchronize(ax));
        std::memcpy(out->rows, c->h_rows.p, row_bytes);
        std::memcpy(out->mask_bits, c->h_rows.p + bit_at, bit_bytes);
        return 0;
    }
    HIPCHK(hipMemcpyAsync(out->rows, c->rows.p, row_bytes, hipMemcpyDeviceToHost, ax));
    HIPCHK(hipMemcpyAsync(out->mask, c->mask8.p, (size_t)nd, hipMemcpyDeviceToHost, ax));
    HIPCHK(hipStreamSynchronize(ax));
    return 0;
}

int ccdgpu_fetch_rows(ccdgpu_ctx *c, int32_t chip, int32_t cx, int32_t cy, int32_t width, ccdgpu_rows *out) {
    if (!c || !out) return fail(CCDGPU_EINVAL, "NULL argument");
    if (chip < 0 || chip >= c->shape.n_chips()) {
        std::memset(out, 0, sizeof(*out));
        return fail(CCDGPU_EINVAL, "chip index out of range");
    }
    return fetch_rows_range(c, chip, chip + 1, &cx, &cy, width, out, false);
}

int ccdgpu_fetch_batch_rows(ccdgpu_ctx *c, const int32_t *cx, const int32_t *cy, int32_t width, ccdgpu_rows *out) {
    if (!c || !out || !cx || !cy) return fail(CCDGPU_EINVAL, "NULL argument");
    if (c->shape.n_chips() <= 0) {
        std::memset(out, 0, sizeof(*out));
        return fail(CCDGPU_EINVAL, "no completed run to fetch");
    }
    return fetch_rows_range(c, 0, c->shape.n_chips(), cx, cy, width, out, true);
}

int ccdgpu_fetch_batch_rows_into(ccdgpu_ctx *c, const int32_t *cx, const int32_t *cy, int32_t width, int64_t *row_offsets,
                                 int64_t offsets_cap, ccdgpu_row *rows, int64_t rows_cap, uint32_t *mask_bits,
                                 int64_t mask_cap, int64_t *n_rows) {
    if (!c || !cx || !cy || !row_offsets || !rows || !mask_bits || !n_rows) return fail(CCDGPU_EINVAL, "NULL argument");
    *n_rows = 0;
    if (!c->ran || c->shape.n_chips() <= 0) return fail(CCDGPU_EINVAL, "no completed run to fetch");
    if (width <= 0) return fail(CCDGPU_EINVAL, "width must be > 0");
    HIPCHK(hipSetDevice(c->device));
    const Shape &sh = c->shape;
    const int32_t nc = sh.n_chips();
    const int64_t np = sh.pix_off[nc];
    // rows per pixel = max(1, segments), from the segment offsets already on the host
    int64_t nr = 0;
    for (int64_t i = 0; i < np; ++i) nr += std::max<int64_t>(1, c->h_offsets[i + 1] - c->h_offsets[i]);
    *n_rows = nr;
    const size_t nbits = (size_t)np * c->mask_words;
    if (offsets_cap < np + 1 || rows_cap < nr || mask_cap < (int64_t)nbits)
        return fail(CCDGPU_EINVAL, "fetch_batch_rows_into: buffers too small (need " + std::to_string(np + 1) +
                                       " offsets, " + std::to_string(nr) + " rows, " + std::to_string(nbits) + " mask words)");
    int rc;
    if ((rc = c->rows.ensure((size_t)(nr > 0 ? nr : 1))) || (rc = c->row_off.ensure(np + 1)) || (rc = c->seg_off1.ensure(np + 1)))
        return rc;
    const size_t ob = sizeof(int64_t) * (size_t)(np + 1);
    if ((rc = c->h_fo.ensure(2 * ob))) return rc;
    int64_t *soff = reinterpret_cast<int64_t *>(c->h_fo.p), *roff = soff + (np + 1);
    const int64_t s0 = c->h_offsets[0];
    roff[0] = 0;
    for (int64_t i = 0; i <= np; ++i) soff[i] = c->h_offsets[i] - s0;
    for (int64_t i = 0; i < np; ++i) roff[i + 1] = roff[i] + std::max<int64_t>(1, soff[i + 1] - soff[i]);
    hipStream_t ax = c->aux;
    HIPCHK(hipMemcpyAsync(c->seg_off1.p, soff, ob, hipMemcpyHostToDevice, ax));
    HIPCHK(hipMemcpyAsync(c->row_off.p, roff, ob, hipMemcpyHostToDevice, ax));
    for (int32_t ch = 0; ch < nc; ++ch) {
        const int64_t q = sh.pix_off[ch];
        if (ccdk_pack_rows(c->csr.p + s0, c->seg_off1.p + q, c->row_off.p + q, c->mask.p + (size_t)q * c->mask_words,
                           c->mask_words, sh.npix[ch], sh.nobs[ch], cx[ch], cy[ch], width, c->rows.p, nullptr, nullptr,
                           INT64_MAX, INT64_MAX, ax))
            return fail(CCDGPU_EHIP, "row packing launch failed");
    }
    // straight into the caller's buffers (DMA when they are pinned: ccdgpu_host_alloc)
    if (nr > 0) HIPCHK(hipMemcpyAsync(rows, c->rows.p, sizeof(ccdgpu_row) * (size_t)nr, hipMemcpyDeviceToHost, ax));
    if (nbits > 0) HIPCHK(hipMemcpyAsync(mask_bits, c->mask.p, sizeof(uint32_t) * nbits, hipMemcpyDeviceToHost, ax));
    std::memcpy(row_offsets, roff, ob);
    HIPCHK(hipStreamSynchronize(ax));
    return 0;
}

void ccdgpu_rows_free(ccdgpu_rows *r) {
    if (!r) return;
    std::free(r->row_offsets);
    std::free(r->rows);
    std::free(r->mask);
    std::free(r->mask_bits);
    std::memset(r, 0, sizeof(*r));
}

int ccdgpu_fetch_staged(ccdgpu_ctx *c, int32_t chip, ccdgpu_result *out) {
    if (!c || !out) return fail(CCDGPU_EINVAL, "NULL argument");
    return fetch_chip(c, chip, out);
}

int ccdgpu_detect_batch(ccdgpu_ctx *c, const ccdgpu_params *params, int32_t n_pix, int32_t n_obs,
                        const int64_t *dates, const int16_t *spectra, const uint16_t *qa, ccdgpu_result *out) {
    if (!out) return fail(CCDGPU_EINVAL, "NULL result");
    std::memset(out, 0, sizeof(*out));
    auto t0 = std::chrono::steady_clock::now();
    int rc = ccdgpu_stage(c, params, 1, n_pix, n_obs, dates, spectra, qa);
    if (rc) return rc;
    double ks = 0;
    rc = ccdgpu_run_staged(c, &ks);
    if (rc && rc != CCDGPU_EQA) return rc;
    const int rc_qa = rc;
    const std::string qa_msg = g_err;
    rc = fetch_chip(c, 0, out);
    if (rc) return rc;
    out->seconds_kernel = ks;
    out->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc_qa) g_err = qa_msg;
    return rc_qa;
}

void ccdgpu_result_free(ccdgpu_result *r) {
    if (!r) return;
    std::free(r->seg_offsets);
    std::free(r->segments);
    std::free(r->mask_bits);
    std::free(r->procedure);
    std::free(r->probs);
    std::free(r->sorted_dates);
    std::free(r->sort_index);
    std::memset(r, 0, sizeof(*r));
}

// ---- random-forest classification of segment rows (include/ccdgpu.h; kernels in ccd_forest.hip)

// The checks of ccdgpu_forest_check, and the forest's depth (branches from a root to its deepest
// leaf).  Children have larger indices than their parents, so one pass in index order carries
// the depth down from the roots.
static int forest_validate(const ccdgpu_forest *f, int32_t *max_depth) {
    if (!f) return fail(CCDGPU_EINVAL, "forest is NULL");
    if (f->n_trees < 1) return fail(CCDGPU_EINVAL, "forest: n_trees must be >= 1, got " + std::to_string(f->n_trees));
    if (f->n_nodes < 1) return fail(CCDGPU_EINVAL, "forest: n_nodes must be >= 1, got " + std::to_string(f->n_nodes));
    if (f->n_features < 1 || f->n_features > CCDGPU_FOREST_MAX_FEATURES)
        return fail(CCDGPU_EINVAL, "forest: n_features must be in [1, " + std::to_string(CCDGPU_FOREST_MAX_FEATURES) + "], got " +
                                       std::to_string(f->n_features));
    if (f->n_classes < 1 || f->n_classes > CCDGPU_FOREST_MAX_CLASSES)
        return fail(CCDGPU_EINVAL, "forest: n_classes must be in [1, " + std::to_string(CCDGPU_FOREST_MAX_CLASSES) + "], got " +
                                       std::to_string(f->n_classes));
    if (!f->root || !f->feature || !f->threshold || !f->left || !f->right || !f->value)
        return fail(CCDGPU_EINVAL, "forest: NULL array");
    const int32_t nn = f->n_nodes, nc = f->n_classes;
    // depth of a node below its root; -1: not reached from any root; parents counted in `seen`
    std::vector<int32_t> depth((size_t)nn, -1);
    std::vector<unsigned char> seen((size_t)nn, 0);
    for (int32_t t = 0; t < f->n_trees; ++t) {
        const int32_t r = f->root[t];
        if (r < 0 || r >= nn)
            return fail(CCDGPU_EINVAL, "forest: root of tree " + std::to_string(t) + " is " + std::to_string(r) +
                                           ", outside [0, " + std::to_string(nn) + ")");
        if (seen[r]) return fail(CCDGPU_EINVAL, "forest: node " + std::to_string(r) + " is the root of two trees (shared node)");
        seen[r] = 1;
        depth[r] = 0;
    }
    int32_t deepest = 0;
    for (int32_t n = 0; n < nn; ++n) {
        if (f->feature[n] < 0) {
            for (int32_t k = 0; k < nc; ++k)
                if (!std::isfinite(f->value[(size_t)n * nc + k]))
                    return fail(CCDGPU_EINVAL, "forest: leaf " + std::to_string(n) + " has a non-finite value (class " +
                                                   std::to_string(k) + ")");
            if (depth[n] > deepest) deepest = depth[n];
            continue;
        }
        if (f->feature[n] >= f->n_features)
            return fail(CCDGPU_EINVAL, "forest: node " + std::to_string(n) + " tests feature " + std::to_string(f->feature[n]) +
                                           " >= n_features " + std::to_string(f->n_features));
        if (!std::isfinite(f->threshold[n]))
            return fail(CCDGPU_EINVAL, "forest: node " + std::to_string(n) + " has a non-finite threshold");
        const int32_t ch[2] = {f->left[n], f->right[n]};
        for (int32_t side = 0; side < 2; ++side) {
            const int32_t c = ch[side];
            const char *name = side ? "right" : "left";
            if (c < 0 || c >= nn)
                return fail(CCDGPU_EINVAL, "forest: " + std::string(name) + " child of node " + std::to_string(n) + " is " +
                                               std::to_string(c) + ", outside [0, " + std::to_string(nn) + ")");
            if (c <= n)
                return fail(CCDGPU_EINVAL, "forest: " + std::string(name) + " child of node " + std::to_string(n) + " is " +
                                               std::to_string(c) + ", not greater than its parent's index");
            if (seen[c]) return fail(CCDGPU_EINVAL, "forest: node " + std::to_string(c) + " has two parents (shared node)");
            seen[c] = 1;
            if (depth[n] >= 0) depth[c] = depth[n] + 1;
        }
    }
    if (max_depth) *max_depth = deepest;
    return 0;
}

int ccdgpu_forest_check(const ccdgpu_forest *f) { return forest_validate(f, nullptr); }

int ccdgpu_forest_depth(const ccdgpu_forest *f, int32_t *max_depth) {
    if (!max_depth) return fail(CCDGPU_EINVAL, "NULL argument");
    *max_depth = 0;
    return forest_validate(f, max_depth);
}

int ccdgpu_forest_clear(ccdgpu_ctx *c) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    (void)hipSetDevice(c->device);
    c->has_forest = false;
    c->forest = CcdForestDev{};
    c->f_pool.release();
    c->f_tree_off.release();
    c->f_chunk_first.release();
    return 0;
}

// The device form of a checked forest (ccd_device.h): per tree one blob, nodes breadth-first so
// that the children of a node are adjacent, the leaves' class vectors behind the nodes; then the
// chunks: runs of whole trees that fit `cap` bytes, a larger tree alone.
static int forest_build(const ccdgpu_forest *f, int32_t cap, std::vector<unsigned char> &pool, std::vector<int64_t> &tree_off,
                        std::vector<int32_t> &chunk_first) {
    const int32_t nt = f->n_trees, nc = f->n_classes;
    tree_off.assign((size_t)nt + 1, 0);
    pool.clear();
    std::vector<int32_t> order;
    for (int32_t t = 0; t < nt; ++t) {
        order.assign(1, f->root[t]);
        size_t leaves = 0;
        for (size_t i = 0; i < order.size(); ++i) {
            const int32_t n = order[i];
            if (f->feature[n] < 0) {
                ++leaves;
            } else {
                order.push_back(f->left[n]);
                order.push_back(f->right[n]);
            }
        }
        const size_t n_t = order.size();
        const size_t bytes = (n_t * sizeof(CcdForestNode) + leaves * nc * sizeof(double) + 15) & ~(size_t)15;
        if (bytes / 8 >= (size_t)INT32_MAX) return fail(CCDGPU_EINVAL, "forest: tree " + std::to_string(t) + " is too large");
        const size_t at = pool.size();
        pool.resize(at + bytes, 0);
        CcdForestNode *nodes = reinterpret_cast<CcdForestNode *>(pool.data() + at);
        double *vals = reinterpret_cast<double *>(pool.data() + at);
        size_t next = 1, leaf = 0;
        for (size_t i = 0; i < n_t; ++i) {
            const int32_t n = order[i];
            if (f->feature[n] < 0) {
                const size_t v = n_t * sizeof(CcdForestNode) / sizeof(double) + leaf * nc;
                nodes[i].threshold = 0.0;
                nodes[i].feature = -1;
                nodes[i].left = (int32_t)v;
                std::memcpy(vals + v, f->value + (size_t)n * nc, sizeof(double) * nc);
                ++leaf;
            } else {
                nodes[i].threshold = f->threshold[n];
                nodes[i].feature = f->feature[n];
                nodes[i].left = (int32_t)next;
                next += 2;
            }
        }
        tree_off[t + 1] = (int64_t)pool.size();
    }
    chunk_first.assign(1, 0);
    for (int32_t t = 0; t < nt;) {
        int32_t e = t + 1;
        if (tree_off[e] - tree_off[t] <= cap)
            while (e < nt && tree_off[e + 1] - tree_off[t] <= cap) ++e;
        chunk_first.push_back(e);
        t = e;
    }
    return 0;
}

int ccdgpu_forest_set(ccdgpu_ctx *c, const ccdgpu_forest *f) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    int32_t max_depth = 0;
    int rc = forest_validate(f, &max_depth);
    if (rc) return rc;
    const int32_t nc = f->n_classes;
    const int32_t cap = ccdk_forest_chunk_cap(f->n_features);
    std::vector<unsigned char> pool;
    std::vector<int64_t> tree_off;
    std::vector<int32_t> chunk_first;
    if ((rc = forest_build(f, cap, pool, tree_off, chunk_first))) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->aux));
    c->has_forest = false;
    if ((rc = c->f_pool.ensure(pool.size())) || (rc = c->f_tree_off.ensure(tree_off.size())) ||
        (rc = c->f_chunk_first.ensure(chunk_first.size())))
        return rc;
    HIPCHK(hipMemcpy(c->f_pool.p, pool.data(), pool.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->f_tree_off.p, tree_off.data(), sizeof(int64_t) * tree_off.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->f_chunk_first.p, chunk_first.data(), sizeof(int32_t) * chunk_first.size(), hipMemcpyHostToDevice));
    for (auto &e : c->f_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    c->forest.pool = c->f_pool.p;
    c->forest.tree_off = c->f_tree_off.p;
    c->forest.chunk_first = c->f_chunk_first.p;
    c->forest.n_chunks = (int32_t)chunk_first.size() - 1;
    c->forest.n_features = f->n_features;
    c->forest.n_classes = nc;
    c->forest.max_depth = max_depth;
    c->forest.threads = ccdk_forest_threads(f->n_features);
    c->forest.chunk_cap = cap;
    c->has_forest = true;
    return 0;
}

// rows a classification keeps on the device at a time (the host-matrix path goes slab by slab;
// a row's result does not depend on its slab)
static const int64_t FOREST_SLAB = (int64_t)1 << 20;

int ccdgpu_classify(ccdgpu_ctx *c, const double *features, int64_t n_rows, float *rfrawp, double *kernel_seconds) {
    if (kernel_seconds) *kernel_seconds = 0.0;
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (!c->has_forest) return fail(CCDGPU_EINVAL, "no forest set (ccdgpu_forest_set)");
    if (c->pending) return fail(CCDGPU_EINVAL, "a detection begun with ccdgpu_run_slot_begin is not finished");
    if (n_rows < 0) return fail(CCDGPU_EINVAL, "n_rows must be >= 0");
    if (n_rows == 0) return 0;
    if (!features || !rfrawp) return fail(CCDGPU_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    const int64_t nf = c->forest.n_features, nc = c->forest.n_classes;
    const int64_t slab = std::min(n_rows, FOREST_SLAB);
    int rc;
    if ((rc = c->f_x.ensure((size_t)(slab * nf))) || (rc = c->f_out.ensure((size_t)(slab * nc)))) return rc;
    hipStream_t ax = c->aux;
    double secs = 0.0;
    for (int64_t r0 = 0; r0 < n_rows; r0 += slab) {
        const int64_t n = std::min(slab, n_rows - r0);
        HIPCHK(hipMemcpyAsync(c->f_x.p, features + r0 * nf, sizeof(double) * (size_t)(n * nf), hipMemcpyHostToDevice, ax));
        HIPCHK(hipEventRecord(c->f_ev[0], ax));
        if (ccdk_forest_classify(&c->forest, c->f_x.p, nullptr, n, c->f_out.p, ax)) {
            (void)hipStreamSynchronize(ax);
            return fail(CCDGPU_EHIP, "forest kernel launch failed");
        }
        HIPCHK(hipEventRecord(c->f_ev[1], ax));
        HIPCHK(hipMemcpyAsync(rfrawp + r0 * nc, c->f_out.p, sizeof(float) * (size_t)(n * nc), hipMemcpyDeviceToHost, ax));
        HIPCHK(hipStreamSynchronize(ax));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->f_ev[0], c->f_ev[1]);
        secs += ms * 1e-3;
    }
    if (kernel_seconds) *kernel_seconds = secs;
    return 0;
}

int ccdgpu_classify_rows(ccdgpu_ctx *c, const double *aux, float *rfrawp, int64_t rows_cap, int64_t *n_rows,
                         double *kernel_seconds) {
    if (kernel_seconds) *kernel_seconds = 0.0;
    if (!n_rows) return fail(CCDGPU_EINVAL, "NULL argument");
    *n_rows = 0;
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (c->pending) return fail(CCDGPU_EINVAL, "a detection begun with ccdgpu_run_slot_begin is not finished");
    if (!c->ran || c->shape.n_chips() <= 0) return fail(CCDGPU_EINVAL, "no completed run to classify");
    // the rows of the run, as ccdgpu_fetch_batch_rows_into counts them: max(1, segments) per pixel
    const int64_t np = c->shape.total_pix();
    if ((int64_t)c->h_offsets.size() < np + 1) return fail(CCDGPU_EINVAL, "no completed run to classify");
    int64_t nr = 0;
    for (int64_t i = 0; i < np; ++i) nr += std::max<int64_t>(1, c->h_offsets[i + 1] - c->h_offsets[i]);
    *n_rows = nr;
    if (!c->has_forest) return fail(CCDGPU_EINVAL, "no forest set (ccdgpu_forest_set)");
    if (c->forest.n_features != 33)
        return fail(CCDGPU_EINVAL, "classify_rows needs a forest of 33 features (ccdc.features.columns()), this one has " +
                                       std::to_string(c->forest.n_features));
    if (rows_cap < nr)
        return fail(CCDGPU_EINVAL, "classify_rows: buffer too small (need " + std::to_string(nr) + " rows)");
    if (!aux || !rfrawp) return fail(CCDGPU_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    const int64_t nc = c->forest.n_classes;
    const int64_t s0 = c->h_offsets[0], n_seg = c->h_offsets[np] - s0;
    int rc;
    if ((rc = c->row_off.ensure(np + 1)) || (rc = c->seg_off1.ensure(np + 1)) || (rc = c->f_aux.ensure((size_t)np * 5)) ||
        (rc = c->f_x.ensure((size_t)nr * 33)) || (rc = c->f_skip.ensure((size_t)nr)) || (rc = c->f_out.ensure((size_t)(nr * nc))))
        return rc;
    const size_t ob = sizeof(int64_t) * (size_t)(np + 1);
    if ((rc = c->h_fo.ensure(2 * ob))) return rc;
    int64_t *soff = reinterpret_cast<int64_t *>(c->h_fo.p), *roff = soff + (np + 1);
    roff[0] = 0;
    for (int64_t i = 0; i <= np; ++i) soff[i] = c->h_offsets[i] - s0;
    for (int64_t i = 0; i < np; ++i) roff[i + 1] = roff[i] + std::max<int64_t>(1, soff[i + 1] - soff[i]);
    hipStream_t ax = c->aux;
    HIPCHK(hipMemcpyAsync(c->seg_off1.p, soff, ob, hipMemcpyHostToDevice, ax));
    HIPCHK(hipMemcpyAsync(c->row_off.p, roff, ob, hipMemcpyHostToDevice, ax));
    HIPCHK(hipMemcpyAsync(c->f_aux.p, aux, sizeof(double) * (size_t)np * 5, hipMemcpyHostToDevice, ax));
    HIPCHK(hipEventRecord(c->f_ev[0], ax));
    if (ccdk_forest_gather(c->csr.p + s0, c->seg_off1.p, c->row_off.p, c->f_aux.p, np, n_seg, nr, c->f_x.p, c->f_skip.p, ax) ||
        ccdk_forest_classify(&c->forest, c->f_x.p, c->f_skip.p, nr, c->f_out.p, ax)) {
        (void)hipStreamSynchronize(ax);
        return fail(CCDGPU_EHIP, "forest kernel launch failed");
    }
    HIPCHK(hipEventRecord(c->f_ev[1], ax));
    HIPCHK(hipMemcpyAsync(rfrawp, c->f_out.p, sizeof(float) * (size_t)(nr * nc), hipMemcpyDeviceToHost, ax));
    HIPCHK(hipStreamSynchronize(ax));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->f_ev[0], c->f_ev[1]);
    if (kernel_seconds) *kernel_seconds = ms * 1e-3;
    return 0;
}

// ---- prediction of band values from segment models (include/ccdgpu.h; kernels in ccd_predict.hip)

// device bytes of a slab's output when the context names no pixel count
static const int64_t PREDICT_SLAB_BYTES = (int64_t)256 << 20;

static int predict_check_dates(int64_t n_dates, const int64_t *dates, double avg_days_yr) {
    if (n_dates < 0) return fail(CCDGPU_EINVAL, "predict: n_dates must be >= 0, got " + std::to_string(n_dates));
    if (n_dates > INT32_MAX) return fail(CCDGPU_EINVAL, "predict: n_dates must be < 2^31, got " + std::to_string(n_dates));
    if (n_dates > 0 && !dates) return fail(CCDGPU_EINVAL, "predict: dates is NULL");
    if (!std::isfinite(avg_days_yr) || !(avg_days_yr > 0.0))
        return fail(CCDGPU_EINVAL, "predict: avg_days_yr must be finite and > 0, got " + std::to_string(avg_days_yr));
    for (int64_t i = 0; i < n_dates; ++i)
        if (dates[i] < 1 || dates[i] > CCDGPU_PREDICT_MAX_DATE)
            return fail(CCDGPU_EINVAL, "predict: dates[" + std::to_string(i) + "] = " + std::to_string(dates[i]) +
                                           " is outside 1 .. " + std::to_string(CCDGPU_PREDICT_MAX_DATE));
    return 0;
}

static int predict_check_modes(int32_t cover, int32_t dtype) {
    if (cover != CCDGPU_COVER_SPAN && cover != CCDGPU_COVER_EXTEND)
        return fail(CCDGPU_EINVAL, "predict: unknown cover " + std::to_string(cover));
    if (dtype != CCDGPU_PREDICT_F32 && dtype != CCDGPU_PREDICT_I16)
        return fail(CCDGPU_EINVAL, "predict: unknown dtype " + std::to_string(dtype));
    return 0;
}

int ccdgpu_predict_check(int64_t n_pix, const int64_t *row_offsets, int64_t n_rows, const ccdgpu_row *rows, int64_t n_dates,
                         const int64_t *dates, double avg_days_yr, int32_t cover, int32_t dtype) {
    if (n_pix < 0) return fail(CCDGPU_EINVAL, "predict: n_pix must be >= 0, got " + std::to_string(n_pix));
    if (n_rows < 0) return fail(CCDGPU_EINVAL, "predict: n_rows must be >= 0, got " + std::to_string(n_rows));
    if (!row_offsets) return fail(CCDGPU_EINVAL, "predict: row_offsets is NULL");
    if (n_rows > 0 && !rows) return fail(CCDGPU_EINVAL, "predict: rows is NULL");
    if (row_offsets[0] != 0)
        return fail(CCDGPU_EINVAL, "predict: row_offsets[0] must be 0, got " + std::to_string(row_offsets[0]));
    for (int64_t p = 0; p < n_pix; ++p)
        if (row_offsets[p + 1] < row_offsets[p])
            return fail(CCDGPU_EINVAL, "predict: row_offsets decrease at pixel " + std::to_string(p) + " (" +
                                           std::to_string(row_offsets[p]) + " -> " + std::to_string(row_offsets[p + 1]) + ")");
    if (row_offsets[n_pix] != n_rows)
        return fail(CCDGPU_EINVAL, "predict: row_offsets[n_pix] is " + std::to_string(row_offsets[n_pix]) + ", n_rows is " +
                                       std::to_string(n_rows));
    int rc = predict_check_dates(n_dates, dates, avg_days_yr);
    if (rc) return rc;
    return predict_check_modes(cover, dtype);
}

static int predict_events(ccdgpu_ctx *c) {
    for (auto &e : c->p_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    return 0;
}

// Both paths, slab by slab over whole pixels: pixel p has the models h_off[p] .. h_off[p + 1] of the
// host table h_rows (uploaded per slab) or, with h_rows NULL, of the device segments d_seg [n_seg].
// A slab's values come back as 7 copies, one per band, into the caller's [7][n_pix][n_dates].
static int predict_run(ccdgpu_ctx *c, const ccdgpu_row *h_rows, const ccdgpu_segment *d_seg, int64_t n_seg,
                       const int64_t *h_off, int64_t n_pix, int64_t n_dates, const int64_t *dates, double avg_days_yr,
                       int32_t cover, int32_t dtype, void *out, int32_t *seg_index, double *kernel_seconds) {
    HIPCHK(hipSetDevice(c->device));
    int rc = predict_events(c);
    if (rc) return rc;
    const int64_t esz = dtype == CCDGPU_PREDICT_I16 ? 2 : 4;
    int64_t slab = c->predict_slab_pixels > 0 ? c->predict_slab_pixels
                                              : std::max<int64_t>(1, PREDICT_SLAB_BYTES / (n_dates * (CCDGPU_NBANDS * esz + 4)));
    slab = std::min(slab, std::min(n_pix, ccdk_predict_max_pixels()));
    if ((rc = c->p_dates.ensure((size_t)n_dates)) || (rc = c->p_basis.ensure((size_t)n_dates * 8)) ||
        (rc = c->p_off.ensure((size_t)slab + 1)) || (rc = c->p_out.ensure((size_t)(CCDGPU_NBANDS * slab * n_dates * esz))) ||
        (seg_index && (rc = c->p_idx.ensure((size_t)(slab * n_dates)))))
        return rc;
    hipStream_t ax = c->aux;
    HIPCHK(hipMemcpyAsync(c->p_dates.p, dates, sizeof(int64_t) * (size_t)n_dates, hipMemcpyHostToDevice, ax));
    double secs = 0.0;
    for (int64_t p0 = 0; p0 < n_pix; p0 += slab) {
        const int64_t np = std::min(slab, n_pix - p0);
        const int64_t r0 = h_off[p0], nr = h_off[p0 + np] - r0;
        HIPCHK(hipMemcpyAsync(c->p_off.p, h_off + p0, sizeof(int64_t) * (size_t)(np + 1), hipMemcpyHostToDevice, ax));
        if (h_rows && nr > 0) {
            if ((rc = c->p_rows.ensure((size_t)nr))) {
                (void)hipStreamSynchronize(ax);
                return rc;
            }
            HIPCHK(hipMemcpyAsync(c->p_rows.p, h_rows + r0, sizeof(ccdgpu_row) * (size_t)nr, hipMemcpyHostToDevice, ax));
        }
        HIPCHK(hipEventRecord(c->p_ev[0], ax));
        int bad = p0 == 0 ? ccdk_predict_basis(c->p_dates.p, n_dates, avg_days_yr, c->p_basis.p, ax) : 0;
        int32_t *idx = seg_index ? c->p_idx.p : nullptr;
        if (!bad)
            bad = h_rows ? ccdk_predict_rows(c->p_rows.p, c->p_off.p, r0, nr, np, c->p_dates.p, c->p_basis.p, n_dates, cover, dtype,
                                             c->p_out.p, idx, ax)
                         : ccdk_predict_segments(d_seg, c->p_off.p, 0, n_seg, np, c->p_dates.p, c->p_basis.p, n_dates, cover,
                                                 dtype, c->p_out.p, idx, ax);
        if (bad) {
            (void)hipStreamSynchronize(ax);
            return fail(CCDGPU_EHIP, "predict kernel launch failed");
        }
        HIPCHK(hipEventRecord(c->p_ev[1], ax));
        const size_t band = (size_t)(np * n_dates * esz);
        for (int b = 0; b < CCDGPU_NBANDS; ++b)
            HIPCHK(hipMemcpyAsync(static_cast<unsigned char *>(out) + ((size_t)b * n_pix + p0) * n_dates * esz,
                                  c->p_out.p + (size_t)b * band, band, hipMemcpyDeviceToHost, ax));
        if (seg_index)
            HIPCHK(hipMemcpyAsync(seg_index + p0 * n_dates, c->p_idx.p, sizeof(int32_t) * (size_t)(np * n_dates),
                                  hipMemcpyDeviceToHost, ax));
        HIPCHK(hipStreamSynchronize(ax));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->p_ev[0], c->p_ev[1]);
        secs += ms * 1e-3;
    }
    if (kernel_seconds) *kernel_seconds = secs;
    return 0;
}

int ccdgpu_predict(ccdgpu_ctx *c, int64_t n_pix, const int64_t *row_offsets, const ccdgpu_row *rows, int64_t n_dates,
                   const int64_t *dates, double avg_days_yr, int32_t cover, int32_t dtype, void *out, int32_t *seg_index,
                   double *kernel_seconds) {
    if (kernel_seconds) *kernel_seconds = 0.0;
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (c->pending) return fail(CCDGPU_EINVAL, "a detection begun with ccdgpu_run_slot_begin is not finished");
    if (n_pix < 0) return fail(CCDGPU_EINVAL, "predict: n_pix must be >= 0, got " + std::to_string(n_pix));
    if (!row_offsets) return fail(CCDGPU_EINVAL, "predict: row_offsets is NULL");
    int rc = ccdgpu_predict_check(n_pix, row_offsets, row_offsets[n_pix], rows, n_dates, dates, avg_days_yr, cover, dtype);
    if (rc) return rc;
    if (n_pix == 0 || n_dates == 0) return 0;
    if (!out) return fail(CCDGPU_EINVAL, "predict: out is NULL");
    return predict_run(c, rows, nullptr, 0, row_offsets, n_pix, n_dates, dates, avg_days_yr, cover, dtype, out, seg_index,
                       kernel_seconds);
}

int ccdgpu_predict_rows(ccdgpu_ctx *c, int32_t chip, int64_t n_dates, const int64_t *dates, double avg_days_yr, int32_t cover,
                        int32_t dtype, void *out, int32_t *seg_index, double *kernel_seconds) {
    if (kernel_seconds) *kernel_seconds = 0.0;
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (c->pending) return fail(CCDGPU_EINVAL, "a detection begun with ccdgpu_run_slot_begin is not finished");
    if (!c->ran || c->shape.n_chips() <= 0) return fail(CCDGPU_EINVAL, "no completed run to predict from");
    const int64_t total = c->shape.total_pix();
    if ((int64_t)c->h_offsets.size() < total + 1) return fail(CCDGPU_EINVAL, "no completed run to predict from");
    if (chip < 0 || chip >= c->shape.n_chips())
        return fail(CCDGPU_EINVAL, "predict_rows: chip " + std::to_string(chip) + " is outside [0, " +
                                       std::to_string(c->shape.n_chips()) + ")");
    int rc = predict_check_dates(n_dates, dates, avg_days_yr);
    if (rc || (rc = predict_check_modes(cover, dtype))) return rc;
    if (n_dates == 0) return 0;
    if (!out) return fail(CCDGPU_EINVAL, "predict: out is NULL");
    const int64_t p0 = c->shape.pix_off[chip];
    return predict_run(c, nullptr, c->csr.p, c->h_offsets[total], c->h_offsets.data() + p0, c->shape.npix[chip], n_dates, dates,
                       avg_days_yr, cover, dtype, out, seg_index, kernel_seconds);
}

int ccdgpu_coefficient_matrix(ccdgpu_ctx *c, int64_t n_dates, const int64_t *dates, double avg_days_yr, double *basis) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (c->pending) return fail(CCDGPU_EINVAL, "a detection begun with ccdgpu_run_slot_begin is not finished");
    int rc = predict_check_dates(n_dates, dates, avg_days_yr);
    if (rc) return rc;
    if (n_dates == 0) return 0;
    if (!basis) return fail(CCDGPU_EINVAL, "predict: basis is NULL");
    HIPCHK(hipSetDevice(c->device));
    if ((rc = c->p_dates.ensure((size_t)n_dates)) || (rc = c->p_basis.ensure((size_t)n_dates * 8))) return rc;
    hipStream_t ax = c->aux;
    HIPCHK(hipMemcpyAsync(c->p_dates.p, dates, sizeof(int64_t) * (size_t)n_dates, hipMemcpyHostToDevice, ax));
    if (ccdk_predict_basis(c->p_dates.p, n_dates, avg_days_yr, c->p_basis.p, ax)) {
        (void)hipStreamSynchronize(ax);
        return fail(CCDGPU_EHIP, "predict kernel launch failed");
    }
    std::vector<double> b8((size_t)n_dates * 8);
    HIPCHK(hipMemcpyAsync(b8.data(), c->p_basis.p, sizeof(double) * b8.size(), hipMemcpyDeviceToHost, ax));
    HIPCHK(hipStreamSynchronize(ax));
    for (int64_t i = 0; i < n_dates; ++i) std::memcpy(basis + i * 7, b8.data() + i * 8, sizeof(double) * 7);
    return 0;
}

}  // extern "C"
