/* ccdgpu.h -- C-ABI of libccdgpu.so: MI355X (gfx950) CCDC change detection.
 *
 * Drop-in replacement for the per-pixel call the reference makes at
 *     ccdc/pyccd.py:168   ccdresult = ccd.detect(**second(timeseries))
 * (lcmap-pyccd 2018.03.12.dev-ncompare.b2, setup.py:32) over the records that
 *     ccdc/timeseries.py:92-126   (merlin.create -> ((cx,cy,px,py), {dates, blues..thermals, qas}))
 * builds.  One call processes a batch of pixels that share one acquisition-date vector (a chip
 * or part of one, as merlin builds them per chip).  The Python side (lcmap-firebird_amd/ccd,
 * lcmap-firebird_amd/ccdc/pyccd.py) binds these symbols with ctypes; INTEGRATION.md shows the
 * binding.  Plain C types only; no C++ or torch types cross this boundary.
 *
 * Errors: every entry point returns 0 on success or a negative CCDGPU_E* code; the message of the
 * last failure on the calling thread is ccdgpu_last_error().  An unsupported bit-packed QA value
 * is CCDGPU_EQA -- the analogue of pyccd's ValueError from qa.qabitval -- and the offending
 * pixel is reported in ccdgpu_result.error_pixel.
 */
#ifndef CCDGPU_H
#define CCDGPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CCDGPU_OK 0
#define CCDGPU_EINVAL (-1)   /* bad argument / size                                    */
#define CCDGPU_EHIP (-2)     /* HIP runtime error (no device, launch failure, ...)     */
#define CCDGPU_EQA (-3)      /* unsupported bit-packed QA value (pyccd ValueError)     */
#define CCDGPU_ENOMEM (-4)   /* device or host allocation failed                       */
#define CCDGPU_EOVERFLOW (-5)/* capacity exceeded (adaptive peek > CCDGPU_MAX_PEEK)    */

#define CCDGPU_NBANDS 7      /* blue, green, red, nir, swir1, swir2, thermal            */
#define CCDGPU_MAX_OBS 4096  /* observations per pixel the kernels accept              */
/* Largest (adaptive) look-ahead window.  The ncompare peek is round(16 PEEK_SIZE / median gap)
 * over the filtered, duplicate-free dates, so with the default PEEK_SIZE 6 it never exceeds 96
 * (median gap >= 1 day): every default-parameter pixel is supported.  A configured PEEK_SIZE > 6
 * can push it past 96 on dense dates; that pixel fails the call with CCDGPU_EOVERFLOW. */
#define CCDGPU_MAX_PEEK 96

/* ccd/parameters.yaml defaults; ccdgpu_params_default() fills them. */
typedef struct ccdgpu_params {
    int32_t meow_size;          /* 12   MEOW_SIZE                                       */
    int32_t peek_size;          /* 6    PEEK_SIZE (default; ncompare may enlarge it)     */
    int32_t day_delta;          /* 365  DAY_DELTA                                        */
    int32_t coef_min, coef_mid, coef_max; /* 4 / 6 / 8                                    */
    int32_t num_obs_factor;     /* 3                                                     */
    uint32_t detection_bands;   /* bit mask, default bands 1..5 = 0x3E                   */
    uint32_t tmask_bands;       /* bit mask, default bands 1 and 4 = 0x12                */
    int32_t lasso_max_iter;     /* 1000                                                  */
    int32_t thermal_min, thermal_max; /* -9320 / 7070 (deg C x 100)                        */
    int32_t median_green_filter;/* 400                                                   */
    int32_t curve_qa_start, curve_qa_end, curve_qa_insuf_clear, curve_qa_persist_snow; /* 14/24/44/54 */
    int32_t qa_fill, qa_clear, qa_water, qa_shadow, qa_snow, qa_cloud; /* bit offsets 0..5 */
    int32_t qa_cirrus1, qa_cirrus2, qa_occlusion;                      /* 8, 9, 10         */
    int32_t qa_bitpacked;       /* 1: qas are PIXELQA bit fields; 0: already class ids   */
    int32_t adaptive_peek;      /* 1: "ncompare" density-adaptive peek + threshold        */
    int32_t rmse_dof;           /* 1: rmse denominator n - num_coefficients              */
    int32_t kelvin_to_celsius;  /* 1: standard procedure converts thermal (int16 wrap)   */
    double avg_days_yr;         /* 365.2425                                              */
    double change_probability;  /* 0.99                                                  */
    double change_threshold;    /* chi2.ppf(0.99, 5)                                     */
    double outlier_threshold;   /* chi2.ppf(0.999999, 5)                                 */
    double t_const;             /* 4.42 Tmask                                            */
    double lasso_alpha;         /* 1.0 (sklearn Lasso alpha; l1 = alpha * n_samples)     */
    double lasso_tol;           /* 1e-4                                                  */
    double clear_pct_threshold; /* 0.25                                                  */
    double snow_pct_threshold;  /* 0.75                                                  */
    /* tie order of the date sort (ccd/__init__.py detect) and of find_closest_doy
       (change.py): 0 = numpy's argsort kind='quicksort' as the pinned reference image ran it
       (numpy < 1.17 introsort-free aquicksort), 1 = stable (ties by position) */
    int32_t argsort_stable;     /* 0                                                     */
    int32_t reserved0;          /* 0                                                     */
} ccdgpu_params;

/* One change model (pyccd change_model dict; ccdc/pyccd.py:106-148 formats it). */
typedef struct ccdgpu_segment {
    int32_t start_day, end_day, break_day; /* proleptic ordinals                       */
    int32_t observation_count;
    int32_t curve_qa;
    int32_t pixel;                          /* pixel index within the batch             */
    double change_probability;
    double magnitude[CCDGPU_NBANDS];
    double rmse[CCDGPU_NBANDS];
    double intercept[CCDGPU_NBANDS];
    double coef[CCDGPU_NBANDS][7];          /* [band][t, cos, sin, cos2, sin2, cos3, sin3] */
} ccdgpu_segment;

enum { CCDGPU_PROC_STANDARD = 0, CCDGPU_PROC_PERMANENT_SNOW = 1, CCDGPU_PROC_INSUFFICIENT_CLEAR = 2 };

/* Results, CSR by pixel.  Owned by the library until ccdgpu_result_free. */
typedef struct ccdgpu_result {
    int32_t n_pix, n_obs;
    int64_t n_seg;
    int64_t *seg_offsets;       /* [n_pix + 1]                                            */
    ccdgpu_segment *segments;   /* [n_seg], pixel-major, in detection order               */
    uint32_t *mask_bits;        /* [n_pix][mask_words] processing_mask, SORTED date order  */
    int32_t mask_words;         /* (n_obs + 31) / 32                                      */
    int32_t *procedure;         /* [n_pix] CCDGPU_PROC_*                                  */
    double *probs;              /* [n_pix][3] cloud, snow, water                          */
    int64_t *sorted_dates;      /* [n_obs] ascending (argsort of the input dates, ties in */
                                /* params.argsort_stable's order)                         */
    int32_t *sort_index;        /* [n_obs] input position of each sorted observation      */
    int32_t error_pixel;        /* first pixel with an unsupported QA value, else -1      */
    double seconds_kernel;      /* device time of the detection kernels (HIP events)      */
    double seconds_total;       /* wall time of the call                                  */
} ccdgpu_result;

/* One row of the reference's segment table with its storage types (ccdc/segment.py:16-55,
 * resources/schema.cql segment; rows of ccdc/pyccd.py:106-148): float columns rounded to
 * float32 as Spark's FloatType cast does, days as proleptic ordinals (ISO text on the host).
 * A pixel without change models has one row of pyccd.default (pyccd.py:99-103): days 1/1/1 and
 * has_model 0, every band / chprob / curqa column null. */
typedef struct ccdgpu_row {
    int32_t px, py;                 /* cx + 30 col, cy - 30 row (test/__init__.py:37)          */
    int32_t sday, eday, bday;
    int32_t curqa;
    int32_t has_model;
    float chprob;
    float mag[CCDGPU_NBANDS], rmse[CCDGPU_NBANDS];
    float coef[CCDGPU_NBANDS][7];
    float intercept[CCDGPU_NBANDS];
} ccdgpu_row;

/* Segment + pixel table rows of one chip.  Owned by the library until ccdgpu_rows_free. */
typedef struct ccdgpu_rows {
    int32_t n_pix, n_obs;
    int64_t n_rows;
    int64_t *row_offsets;       /* [n_pix + 1]                                             */
    ccdgpu_row *rows;           /* [n_rows], pixel-major                                   */
    int8_t *mask;               /* [n_pix][n_obs] processing mask 0/1, sorted date order   */
                                /* (pixel table, resources/schema.cql pixel.mask); NULL    */
                                /* for a batch fetch, which returns mask_bits instead      */
    uint32_t *mask_bits;        /* batch fetch: [n_pix][mask_words] the same mask as bits  */
    int32_t mask_words;         /* (bit i of word i/32 = sorted observation i), 8x smaller */
} ccdgpu_rows;

typedef struct ccdgpu_ctx ccdgpu_ctx;

const char *ccdgpu_version(void);
const char *ccdgpu_last_error(void);
void ccdgpu_params_default(ccdgpu_params *p);

/* Create a context bound to HIP device `device`.  A context is used by one host thread at a
 * time; up to 16 contexts may live in a process, and contexts on the same device run their
 * detections concurrently (each has its own stream, buffers and launch-argument slot), so a
 * second context's launch fills the CUs the first one's launch tail leaves idle. */
int ccdgpu_init(int device, ccdgpu_ctx **ctx);
/* ccdgpu_init with `copy_cus` CUs reserved for everything of the context but the detection kernel
 * -- the encoded upload's decode kernel, the launch's prep, CSR scan and scatter, the row packing
 * and the small copies -- and the rest for the detection kernel; 0 = no reservation
 * (ccdgpu_init: all on one stream).  Persistent detection waves hold every wave slot of their
 * CUs until the launch drains, so with several contexts one context's short kernels otherwise
 * wait for wave slots behind the others' whole detections; the tile driver (ccdc.runner)
 * reserves 8 of 256.  CCDGPU_COPY_CUS in the
 * environment overrides the value.  (No reference counterpart: an execution detail of the
 * pipelined driver that replaces ccdc/pyccd.py:168's per-chip map.) */
int ccdgpu_init_copy_cus(int device, int copy_cus, ccdgpu_ctx **ctx);
int ccdgpu_destroy(ccdgpu_ctx *ctx);
int ccdgpu_device_count(int *count);
/* NUMA node of HIP device `device`'s PCIe attachment (sysfs numa_node of its bus id; -1 when the
 * platform does not say).  The tile driver (ccdc.runner) keeps its host threads and pinned upload
 * buffers on that node, so the chip copies and the DMA reads of them stay on the socket the GPU
 * hangs off.  (No reference counterpart: Spark placed executors, ccdc/core.py:97-108.) */
int ccdgpu_device_numa_node(int device, int *node);
int ccdgpu_synchronize(ccdgpu_ctx *ctx);

/* Host-buffer entry point (the pyccd.detect / ccd.detect path).
 *   dates   [n_obs]                 ordinals, any order (merlin delivers them descending)
 *   spectra [7][n_pix][n_obs]       int16, band-major, observation-contiguous, input order
 *   qa      [n_pix][n_obs]          uint16 bit-packed PIXELQA (or class ids if !qa_bitpacked)
 * Synchronous: H2D, kernels, D2H.  *out must be released with ccdgpu_result_free. */
int ccdgpu_detect_batch(ccdgpu_ctx *ctx, const ccdgpu_params *params, int32_t n_pix, int32_t n_obs,
                        const int64_t *dates, const int16_t *spectra, const uint16_t *qa,
                        ccdgpu_result *out);
void ccdgpu_result_free(ccdgpu_result *out);

/* Device-resident path (tile runner, benchmarks, batched Spark partitions): stage a batch once,
 * run the detection as often as wanted on the resident copy, fetch results separately.
 *
 * A batch is `n_chips` chips -- pixel groups that share one date vector, as merlin builds them
 * per chip (ccdc/timeseries.py:107-115) -- with their own sizes: chip c has n_pix[c] pixels and
 * n_obs[c] observations, so a tile's base-cadence and sidelap chips (and the date groups of a
 * Spark partition) run in one launch.  Their arrays are packed back to back:
 *   dates   chip c at  O_c = sum_{c' < c} n_obs[c']               [n_obs[c]]
 *   spectra chip c at  7 * D_c, D_c = sum_{c' < c} n_pix[c'] n_obs[c']   [7][n_pix[c]][n_obs[c]]
 *   qa      chip c at  D_c                                          [n_pix[c]][n_obs[c]]
 * Pixel p of the batch is pixel p - sum_{c' < c} n_pix[c'] of chip c. */
int ccdgpu_stage_chips(ccdgpu_ctx *ctx, const ccdgpu_params *params, int32_t n_chips, const int32_t *n_pix,
                       const int32_t *n_obs, const int64_t *dates, const int16_t *spectra, const uint16_t *qa);
/* ccdgpu_stage_chips with every chip of shape (n_pix, n_obs). */
int ccdgpu_stage(ccdgpu_ctx *ctx, const ccdgpu_params *params, int32_t n_chips, int32_t n_pix,
                 int32_t n_obs, const int64_t *dates, const int16_t *spectra, const uint16_t *qa);
int ccdgpu_run_staged(ccdgpu_ctx *ctx, double *kernel_seconds);

/* Chip packer: stage a batch straight from the chipmunk wire format (replaces merlin.create's
 * per-pixel pivot and the repartition shuffle of ccdc/timeseries.py:120-125; payloads as in the
 * reference fixture test/data/chip_response.json).  Layer l (0..6 = blues, greens, reds, nirs,
 * swir1s, swir2s, thermals; 7 = pixel QA) of observation o of chip c is the base64 text (standard
 * alphabet, '=' padded) starting at byte text_offsets[(c * n_obs + o) * 8 + l] of `text`; it
 * decodes to n_pix little-endian int16 (uint16 for QA) values in row-major pixel order.  A
 * negative offset is a missing layer: its pixels become fill (-9999, QA 1).  dates as in
 * ccdgpu_stage.  The text is copied to the device, decoded and pivoted there to the
 * [7][n_pix][n_obs] / [n_pix][n_obs] layout; *unpack_seconds (may be NULL) gets the kernel time.
 * CCDGPU_EINVAL for a payload that runs past text_bytes or is not base64. */
int ccdgpu_stage_chipmunk(ccdgpu_ctx *ctx, const ccdgpu_params *params, int32_t n_chips, int32_t n_pix,
                          int32_t n_obs, const int64_t *dates, const char *text, int64_t text_bytes,
                          const int64_t *text_offsets, double *unpack_seconds);

/* Overlapped upload (HIP copy stream): ccdgpu_stage_slot uploads a batch into input slot
 * 0 .. CCDGPU_UPLOAD_SLOTS-1 and returns at once; ccdgpu_run_slot detects the batch of a slot
 * (after its upload) exactly like ccdgpu_run_staged, results fetched with ccdgpu_fetch_staged /
 * ccdgpu_fetch_rows.  The streaming loop  stage_slot(0, b0); for i: { stage_slot((i+1)&1,
 * b_{i+1}); run_slot(i&1); fetch }  overlaps each upload with the previous batch's detection;
 * with S slots up to S-1 uploads can be queued ahead of the running batch (the tile driver keeps
 * two queued, so the PCIe link stays busy while detection and the row fetch run).  Host inputs must stay valid and
 * unchanged until the run_slot of their slot returns; they should be pinned (ccdgpu_host_alloc),
 * or the upload is synchronous.  Each slot keeps the params it was staged with. */
#define CCDGPU_UPLOAD_SLOTS 4
int ccdgpu_host_alloc(size_t bytes, void **ptr);
int ccdgpu_host_free(void *ptr);
int ccdgpu_stage_slot_chips(ccdgpu_ctx *ctx, int32_t slot, const ccdgpu_params *params, int32_t n_chips,
                            const int32_t *n_pix, const int32_t *n_obs, const int64_t *dates, const int16_t *spectra,
                            const uint16_t *qa);
int ccdgpu_stage_slot(ccdgpu_ctx *ctx, int32_t slot, const ccdgpu_params *params, int32_t n_chips, int32_t n_pix,
                      int32_t n_obs, const int64_t *dates, const int16_t *spectra, const uint16_t *qa);
int ccdgpu_run_slot(ccdgpu_ctx *ctx, int32_t slot, double *kernel_seconds);
/* ccdgpu_run_slot in two halves, so the calling thread can stage further slots while the
 * detection runs: _begin launches it and returns at once, ccdgpu_run_query returns 1 once it has
 * completed (0 while it runs; 1 with nothing begun), _end waits for it and does the rest of
 * ccdgpu_run_slot (status, CSR of the segments; same return codes).  Between _begin and _end only
 * ccdgpu_stage_slot* of other slots and ccdgpu_run_query may be called on the context.  The tile
 * driver (ccdc.runner) stages the batches its fetch thread finishes during the detection. */
int ccdgpu_run_slot_begin(ccdgpu_ctx *ctx, int32_t slot);
int ccdgpu_run_query(ccdgpu_ctx *ctx);
int ccdgpu_run_slot_end(ccdgpu_ctx *ctx, double *kernel_seconds);
/* The split run with the batch's rows in the same device chain (the tile driver's path; rows as
 * ccdgpu_fetch_batch_rows_into gives them, chip c at (cx[c], cy[c])): _begin_rows enqueues the
 * detection and behind it the CSR, the row packing and the copies of the row offsets
 * [total_pixels + 1], the rows (up to rows_cap) and the mask words [total_pixels][mask_words]
 * into the caller's buffers (pinned: ccdgpu_host_alloc), then returns; _end_rows waits once for
 * the whole chain and returns what ccdgpu_run_slot_end returns, with the row count in *n_rows.
 * More rows than rows_cap: CCDGPU_EOVERFLOW with *n_rows set -- the run is complete and
 * ccdgpu_fetch_batch_rows_into fetches its rows into larger buffers.  rows_cap is also what the
 * chain copies back (the whole rows_cap rows, written or not): pass the rows a batch is expected
 * to hold, not the buffer's room (ccdgpu.RowsBuffers learns it: 1.25 x the highest rows per
 * pixel seen).  The buffers must stay alive and untouched until _end_rows returns;
 * ccdgpu_run_query works as for _begin. */
int ccdgpu_run_slot_begin_rows(ccdgpu_ctx *ctx, int32_t slot, const int32_t *cx, const int32_t *cy, int32_t width,
                               int64_t *row_offsets, int64_t offsets_cap, ccdgpu_row *rows, int64_t rows_cap,
                               uint32_t *mask_bits, int64_t mask_cap);
int ccdgpu_run_slot_end_rows(ccdgpu_ctx *ctx, double *kernel_seconds, int64_t *n_rows);

/* Transport-encoded uploads (no reference counterpart -- the tile path's PCIe link is its bound,
 * DESIGN.md §5).  ccdgpu_encode_chips packs chips given as per-chip pointers (spectra
 * [7][n_pix][n_obs] int16, qa [n_pix][n_obs] uint16, the ccdgpu_stage_chips layout of one chip)
 * into `out` (>= ccdgpu_encoded_bound bytes; pinned for an asynchronous upload) and returns the
 * bytes written (< 0 on bad arguments).  Per chip: an observation whose QA word has any of
 * `drop_bits` set sends no band values (the decoder writes -9999); if it also has any of
 * `strict_bits` (a subset of drop_bits) its 7 bands must all be -9999 or the chip is sent raw --
 * drop_bits = strict_bits = the fill bit is lossless; adding the cloud and shadow bits drops
 * only values the detection never reads (ccd_encode.c); QA words become 4-bit indices into the
 * chip's palette when it has at most 16 distinct words, else the chip is sent raw.  Layout (this
 * text is normative; lcmap-firebird_amd/csrc/ccd_enc_layout.h is its one definition in code, with
 * the byte offsets below asserted at compile time):
 *   int64 n_chips; int64 chip_off[n_chips + 1] (bytes from `out`, 256-aligned);
 *   int64 chip_pix[n_chips + 1] (pixel prefix); chip sections:
 *   header (128 B): int32 mode (0 raw, 1 encoded), n_pix, n_obs, n_pal; uint16 pal[16];
 *                   int64 kept, data_off (the chip's offset in the standard layout), band_stride,
 *                   pix_base; uint32 drop_bits
 *   mode 1: uint32 kept_off[n_pix + 1]; uint8 qa4[n_pix][(n_obs + 1) / 2] (low nibble = even
 *           observation); int16 bands[7][band_stride] (kept observations, pixel-major) -- each
 *           part 16-byte aligned
 *   mode 0: uint16 qa[n_pix][n_obs]; int16 spectra[7][n_pix][n_obs].
 *   mode 2 (bit-packed band runs; only from the _flags encoder with CCDGPU_ENC_PACK): the header
 *           as in mode 1 with mode = 2, band_stride = 0, int64 code_words at byte 88 and int64
 *           exc_total at byte 96; then, each part 16-byte aligned:
 *             uint32 kept_off[n_pix + 1]; uint8 qa4[n_pix][(n_obs + 1) / 2]      (as in mode 1)
 *             run[n_pix][7], 16 bytes each: int16 base; uint16 w; uint32 code_word; uint32 exc_off;
 *                                           uint32 n_exc
 *             uint32 codes[code_words + 1]  (the last word is a zero pad: a decoder may always
 *                                           read word i + 1)
 *             int16 exc[exc_total]
 *           For pixel p and band b the kept values in observation order are v_0 .. v_{k-1},
 *           k = kept_off[p + 1] - kept_off[p].  base = min v (0 when k = 0); r_i = v_i - base in
 *           0 .. 65535 (32-bit arithmetic).  The width w is 0 .. 16:
 *             w = 16      the code is r_i, no escapes;
 *             w = 1 .. 15 the code is r_i if r_i < 2^w - 1, else the escape 2^w - 1 and the raw v_i
 *                         is appended to the run's exception list (in order);
 *             w = 0       only when every r_i is 0: no bits stored.
 *           The encoder's w is canonical: the one that minimises w k + 16 e(w), e(w) = the number
 *           of r_i >= 2^w - 1 for w = 1 .. 15, e(16) = 0, w = 0 eligible only with all values
 *           equal; ties go to the smallest w.  The run's codes take ceil(k w / 32) words from
 *           codes[code_word]: bit j of the run is bit j & 31 of word j >> 5, unused top bits of the
 *           last word 0.  Runs lie back to back in (pixel, band) order, so code_word and exc_off
 *           are prefix sums with totals code_words and exc_total, and the bytes are a pure function
 *           of the input (any thread count, scalar or vector encoder).  A packed batch holds mode
 *           2 and mode 0 (raw fallback) sections only.
 * ccdgpu_stage_slot_encoded uploads such a batch (and the dates) into a slot and decodes it on the
 * device, on the copy stream, into exactly the buffers ccdgpu_stage_slot_chips would fill; run it
 * with ccdgpu_run_slot.  ccdgpu_encode_vector_path: 1 if the encoder uses AVX-512 VBMI2.
 * The _flags forms take CCDGPU_ENC_* flags; flags = 0 is the plain form (same bytes, same bound). */
#define CCDGPU_ENC_PACK 1u   /* encodable chips as mode 2 sections instead of mode 1 */
int64_t ccdgpu_encoded_bound(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs);
int64_t ccdgpu_encode_chips(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs, const int16_t *const *spectra,
                            const uint16_t *const *qa, uint8_t *out, int64_t out_cap, int32_t threads,
                            uint16_t drop_bits, uint16_t strict_bits);
int64_t ccdgpu_encoded_bound_flags(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs, uint32_t flags);
int64_t ccdgpu_encode_chips_flags(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs,
                                  const int16_t *const *spectra, const uint16_t *const *qa, uint8_t *out,
                                  int64_t out_cap, int32_t threads, uint16_t drop_bits, uint16_t strict_bits,
                                  uint32_t flags);
int32_t ccdgpu_encode_vector_path(void);
/* The checks ccdgpu_stage_slot_encoded makes before an encoded batch is uploaded (no device
 * needed): the chip table, every section's header against the chip's shape, every section long
 * enough for its mode's layout, and each encoded section's kept-offset table a run per pixel
 * ending at its kept count.  For a mode 2 section also: every run's w <= 16, its code_word and
 * exc_off equal to the prefix sums of ceil(k w / 32) and n_exc over the runs before it, n_exc <= k,
 * the totals equal to the header's code_words and exc_total, and the section long enough for all
 * five parts including the pad word -- a batch that passes is safe to decode whatever its code bits
 * say; modes 1 and 2 do not share a batch.  0, or CCDGPU_EINVAL with the reason in
 * ccdgpu_last_error(). */
int ccdgpu_encoded_check(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs, const uint8_t *enc,
                         int64_t enc_bytes);
int ccdgpu_stage_slot_encoded(ccdgpu_ctx *ctx, int32_t slot, const ccdgpu_params *params, int32_t n_chips,
                              const int32_t *n_pix, const int32_t *n_obs, const int64_t *dates, const uint8_t *enc,
                              int64_t enc_bytes);

/* Copy the staged pixel inputs back to the host in the ccdgpu_stage_chips layout; either
 * pointer may be NULL. */
int ccdgpu_staged_inputs(ccdgpu_ctx *ctx, int16_t *spectra, uint16_t *qa);
/* CSR result of staged chip `chip` (n_pix / n_obs of that chip). */
int ccdgpu_fetch_staged(ccdgpu_ctx *ctx, int32_t chip, ccdgpu_result *out);

/* Output writer: the segment / pixel table rows of staged chip `chip` of the last run, packed on
 * the device (ccd_rows.hip) for the chip at (cx, cy) with `width` pixels per chip row (100).
 * Replaces the per-segment Python formatting of ccdc/pyccd.py:106-148 + Spark's float cast. */
int ccdgpu_fetch_rows(ccdgpu_ctx *ctx, int32_t chip, int32_t cx, int32_t cy, int32_t width, ccdgpu_rows *out);
/* The same for every chip of the batch in one device pass and one copy (the tile runner's
 * gather): chip c at (cx[c], cy[c]); row_offsets over all pixels of the batch; the masks come
 * back bit-packed (out->mask_bits [n_pix of the batch][out->mask_words], out->mask NULL);
 * out->n_obs is 0 for a multi-chip batch. */
int ccdgpu_fetch_batch_rows(ccdgpu_ctx *ctx, const int32_t *cx, const int32_t *cy, int32_t width, ccdgpu_rows *out);
/* ccdgpu_fetch_batch_rows into the caller's buffers (no library allocation, no host copy of the
 * rows or mask words: with pinned buffers from ccdgpu_host_alloc they arrive by DMA):
 * row_offsets [total_pixels + 1], rows [*n_rows], mask_bits [total_pixels][mask_words].  The
 * row count is set in *n_rows even when a buffer is too small (CCDGPU_EINVAL, nothing fetched:
 * grow and call again).  The tile driver reuses one set of pinned buffers per context. */
int ccdgpu_fetch_batch_rows_into(ccdgpu_ctx *ctx, const int32_t *cx, const int32_t *cy, int32_t width,
                                 int64_t *row_offsets, int64_t offsets_cap, ccdgpu_row *rows, int64_t rows_cap,
                                 uint32_t *mask_bits, int64_t mask_cap, int64_t *n_rows);
void ccdgpu_rows_free(ccdgpu_rows *out);

/* Random-forest classification of segment rows: the `rfrawp` column of the segment table
 * (resources/schema.cql segment.rfrawp; the reference fills it with Spark ML's
 * RandomForestClassificationModel.rawPrediction, ccdc/randomforest.py:25-39, 500 trees).  The
 * forest is imported, or trained on the device (ccdgpu_forest_train, below).
 *
 * A forest is plain arrays over one node pool.  For one row x[n_features]:
 *     raw[:] = 0.0 (double)
 *     for t = 0 .. n_trees-1, in this order:
 *         n = root[t]
 *         while feature[n] >= 0:  n = (x[feature[n]] <= threshold[n]) ? left[n] : right[n]
 *         raw[:] += value[n][:]                       (double adds, in tree order)
 *     out[:] = (float) raw[:]                         (round to nearest)
 * A NaN feature value compares false and goes right.  value[] holds the leaves' normalised class
 * distributions (Spark's rawPrediction sums them); the library does not renormalise.  The result
 * of a row does not depend on how rows are batched or launched. */
#define CCDGPU_FOREST_MAX_FEATURES 64
#define CCDGPU_FOREST_MAX_CLASSES 32
typedef struct ccdgpu_forest {
    int32_t n_trees, n_nodes;
    int32_t n_features;         /* 1 .. CCDGPU_FOREST_MAX_FEATURES                          */
    int32_t n_classes;          /* 1 .. CCDGPU_FOREST_MAX_CLASSES                           */
    const int32_t *root;        /* [n_trees] node index of each tree's root                 */
    const int32_t *feature;     /* [n_nodes] feature tested at the node; < 0 marks a leaf   */
    const double *threshold;    /* [n_nodes]                                                */
    const int32_t *left;        /* [n_nodes] child for x[feature] <= threshold              */
    const int32_t *right;       /* [n_nodes] child otherwise                                */
    const double *value;        /* [n_nodes][n_classes], read at leaves only                */
} ccdgpu_forest;
/* The checks every forest passes before it reaches the device (no device needed).  0, or
 * CCDGPU_EINVAL with the reason in ccdgpu_last_error(): sizes outside the limits; a root or child
 * index outside [0, n_nodes); a child index not strictly greater than its parent's (every walk is
 * then finite; sklearn's and Spark's pre-order numbering satisfy it); a node with two parents (or
 * a root that is also a child or another tree's root); an internal node's feature >= n_features;
 * a non-finite threshold at an internal node; a non-finite leaf value.  ccdgpu_forest_depth does
 * the same and returns the largest number of branches from a root to a leaf. */
int ccdgpu_forest_check(const ccdgpu_forest *f);
int ccdgpu_forest_depth(const ccdgpu_forest *f, int32_t *max_depth);
/* Check `f`, upload it and make it the context's forest (the arrays are not needed afterwards);
 * a previous forest is replaced and freed, ccdgpu_destroy frees it, ccdgpu_forest_clear removes
 * it.  The detection entry points are unaffected by a forest. */
int ccdgpu_forest_set(ccdgpu_ctx *ctx, const ccdgpu_forest *f);
int ccdgpu_forest_clear(ccdgpu_ctx *ctx);
/* Host-matrix path: features [n_rows][n_features] (what ccdc.features.matrix returns) ->
 * rfrawp [n_rows][n_classes].  Synchronous; *kernel_seconds (may be NULL) gets the device time of
 * the forest kernel.  n_rows == 0 succeeds without a launch; CCDGPU_EINVAL with no forest set. */
int ccdgpu_classify(ccdgpu_ctx *ctx, const double *features, int64_t n_rows, float *rfrawp, double *kernel_seconds);
/* Chained path (needs n_features == 33): classify the rows of the context's last completed run,
 * in exactly the order and count ccdgpu_fetch_batch_rows_into returns them, without the rows
 * leaving the device.  aux [total_pixels][5]: dem, aspect, slope, mpw, posidex of each pixel of
 * the batch.  The feature vector of a row is ccdc.features.columns(): mag[0..6], rmse[0..6],
 * coef[b][0] for b = 0..6, intercept[0..6] -- the row's float32 values widened to double -- then
 * the pixel's 5 aux values.  A row with has_model == 0 (pyccd.default's row) is not walked and
 * gets NaN in every class.  *n_rows is always set; with rows_cap too small CCDGPU_EINVAL and
 * nothing is written (grow and call again). */
int ccdgpu_classify_rows(ccdgpu_ctx *ctx, const double *aux, float *rfrawp, int64_t rows_cap, int64_t *n_rows,
                         double *kernel_seconds);

/* Training of the random forest on the device: what the reference does with Spark ML's
 * RandomForestClassifier over features.dataframe (ccdc/randomforest.py:25-39) -- trees grown over
 * binned features, level by level, from per-node class histograms.  Parity with Spark ML itself is
 * not pinned here (no fixture), so the rule below is normative: Spark ML's structure and defaults,
 * its uncertain choices parameters, built only from integer counts and a counter-based hash.  The
 * trained forest is a pure function of the inputs: it does not depend on launch shapes, on how the
 * trees are grouped or on the arrival order of atomic adds; a restatement in numpy is equal array by
 * array.
 *
 * Inputs.  x [n_rows][n_features] double, all finite; labels [n_rows] int32 in 0 .. n_classes-1;
 * per feature f, n_edges[f] strictly increasing finite doubles, packed back to back in `edges`
 * (feature f's start at the sum of n_edges before f) -- a feature with n_edges[f] == 0 is never
 * split; struct ccdgpu_train_params.  Limits: n_rows 1 .. 2^27, n_features 1 ..
 * CCDGPU_FOREST_MAX_FEATURES, n_classes 1 .. CCDGPU_FOREST_MAX_CLASSES, n_edges[f] 0 ..
 * CCDGPU_TRAIN_MAX_EDGES (at most 64 bins), n_trees >= 1 with n_trees (2^(max_depth+1) - 1) < 2^31.
 *
 * Bins.  bin(r,f) = the number of e in feature f's edges with e < x[r][f]; so x <= edges[f][b]
 * holds exactly when bin <= b (the inference walk's own test).
 * Hash.  uint64 arithmetic with wraparound.
 *     mix(z):    z ^= z>>30; z *= 0xBF58476D1CE4E5B9; z ^= z>>27; z *= 0x94D049BB133111EB; z ^= z>>31
 *     fold(z,v): mix(z + 0x9E3779B97F4A7C15 + v)
 *     H(seed,a,b,c) = fold(fold(fold(mix(seed + 0x9E3779B97F4A7C15), a), b), c)
 * Row weights.  w(t,r) of row r in tree t is 1 when bootstrap == 0.  Otherwise a Poisson(1) draw by
 *     inverse CDF on integers: u = H(seed,t,r,0) >> 32; w = the number of k with u >= P[k],
 *     P[k] = floor(2^32 sum_{j<=k} e^-1/j!) for k = 0 .. 12 = CCDGPU_TRAIN_POISSON.  The largest
 *     weight is 13 (hence n_rows <= 2^27: every count fits 32 bits).
 * Nodes.  The root is node 1; the children of node i are 2i (left) and 2i+1.
 * Feature subset of node i of tree t: the m features with the smallest keys H(seed,t,i,1+f), ties
 *     to the lower f; m = features_per_node clamped to n_features, 0 meaning the smallest m with
 *     m*m >= n_features (Spark's sqrt); m == n_features: all of them.
 * Leaf or split.  c_k = the weighted class counts of the node's rows (int64), n = sum c_k,
 *     q = sum c_k^2.  The node is a leaf when its depth equals max_depth, or q == n*n (pure; an
 *     integer test), or n < 2 min_instances_per_node, or no candidate is valid.
 * Candidates.  (f in the subset, b in 0 .. n_edges[f]-1); left counts over the rows with
 *     bin(r,f) <= b.  Valid iff nL >= min_instances_per_node and nR >= min_instances_per_node and
 *     gain >= min_info_gain, with the doubles
 *         score = (double)qL/(double)nL + (double)qR/(double)nR
 *         gain  = (score - (double)q/(double)n)/(double)n
 *     each operation one IEEE operation, no contraction.  The chosen candidate has the largest
 *     score; among equal scores the lowest f, then the lowest b.
 * A chosen split makes the node an internal node of ccdgpu_forest with feature = f and threshold =
 *     edges[f][b]; rows with bin <= b go left.
 * Values.  Every node, internal or leaf, has value[k] = (double)c_k/(double)n.
 * Empty bag.  n == 0 at a tree's root: the call fails with CCDGPU_EINVAL naming the tree.
 * Output.  ccdgpu_forest arrays: trees in order, each tree's nodes in pre-order, left before right
 *     (ccdgpu_forest_check passes by construction). */
#define CCDGPU_TRAIN_MAX_ROWS ((int64_t)1 << 27)
#define CCDGPU_TRAIN_MAX_EDGES 63
#define CCDGPU_TRAIN_MAX_DEPTH 10
#define CCDGPU_TRAIN_POISSON_N 13
#define CCDGPU_TRAIN_POISSON                                                                          \
    { 1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u, 4294609777u,      \
      4294923276u, 4294962463u, 4294966817u, 4294967252u, 4294967292u, 4294967295u }
typedef struct ccdgpu_train_params {
    int32_t n_trees;                /* 500  (randomforest.py:31 numTrees)                        */
    int32_t max_depth;              /* 5    0 .. CCDGPU_TRAIN_MAX_DEPTH (Spark's default)         */
    int32_t features_per_node;      /* 0    0: sqrt; clamped to n_features                       */
    int32_t min_instances_per_node; /* 1    >= 1                                                 */
    double min_info_gain;           /* 0.0  >= 0                                                 */
    int32_t bootstrap;              /* 1    0 or 1                                               */
    int32_t reserved0;              /* 0                                                         */
    uint64_t seed;                  /* 0                                                         */
} ccdgpu_train_params;
void ccdgpu_train_params_default(ccdgpu_train_params *p);
/* The checks a training request passes before anything reaches the device (no device needed).  0, or
 * CCDGPU_EINVAL with the reason in ccdgpu_last_error(), naming the argument and the index: a NULL
 * array; a count outside the limits above; a non-finite x; a label outside 0 .. n_classes-1; an edge
 * that is not finite or not above the one before it; a parameter outside its range. */
int ccdgpu_train_check(const double *x, const int32_t *labels, int64_t n_rows, int32_t n_features, int32_t n_classes,
                       const double *edges, const int32_t *n_edges, const ccdgpu_train_params *params);
/* Check, train and keep the result in the context until the next training or ccdgpu_destroy.
 * Synchronous; *kernel_seconds (may be NULL) gets the device time of the kernels.  The trained forest
 * is state of its own: it does not replace the context's forest (ccdgpu_forest_set with the fetched
 * arrays does), and detection and classification are unaffected by it.  The trees are grown in
 * groups sized by a device-memory budget (CCDGPU_TRAIN_GROUP_TREES in the environment, a test knob,
 * fixes the group size); the result does not depend on the grouping.  Refused with CCDGPU_EINVAL
 * while a detection begun with ccdgpu_run_slot_begin is not finished. */
int ccdgpu_forest_train(ccdgpu_ctx *ctx, const double *x, const int32_t *labels, int64_t n_rows, int32_t n_features,
                        int32_t n_classes, const double *edges, const int32_t *n_edges, const ccdgpu_train_params *params,
                        double *kernel_seconds);
/* The trained forest's tree and node counts (CCDGPU_EINVAL when nothing has been trained), and its
 * arrays: `into` has n_trees and n_nodes set to those counts and its six pointers at arrays of that
 * size, which are written; n_features and n_classes are set. */
int ccdgpu_trained_size(ccdgpu_ctx *ctx, int32_t *n_trees, int32_t *n_nodes);
int ccdgpu_trained_fetch(ccdgpu_ctx *ctx, ccdgpu_forest *into);

/* The bin edges of training, found on the device: Spark ML's rule for continuous features
 * (RandomForest.findSplitsForContinuousFeature with every row a sample), which
 * ccdc.randomforest.find_splits computes on the host with a sort per column.  The rule is restated
 * here over positions of the sorted column, the form the device computes; the two are equal array by
 * array, so no tolerance is involved.
 *
 * Inputs.  x [n_rows][n_features] double, all finite; max_bins.  Limits: n_rows 0 ..
 * CCDGPU_TRAIN_MAX_ROWS (0 rows: no launch, no edges), n_features 1 .. CCDGPU_FOREST_MAX_FEATURES,
 * max_bins 2 .. CCDGPU_TRAIN_MAX_EDGES + 1.
 *
 * Per feature, over the column's n = n_rows values:
 * Key.  v + 0.0, so that -0.0 and +0.0 are one value.
 * Sorted column.  s[0 .. n-1] is the column in ascending order.
 * Boundary.  A position p in 1 .. n-1 with s[p] != s[p-1].  The boundaries in order are p_1 < p_2 <
 *     .. < p_B, and p_{B+1} = n.  The column has D = B + 1 distinct values.
 * Midpoint of boundary p_i: (s[p_i - 1] + s[p_i]) / 2.0, two IEEE double operations in that order, no
 *     contraction.  An overflow to +-inf is kept (ccdgpu_train_check refuses such an edge later).
 * Few distinct values.  If D - 1 <= max_bins - 1, every boundary's midpoint is a candidate, in order.
 * Many distinct values.  Otherwise stride = (double)n / (double)max_bins and target = stride; for i =
 *     1, 2, .. B in order: if fabs((double)p_i - target) < fabs((double)p_{i+1} - target), the midpoint
 *     of boundary i is a candidate and target += stride.  (p_i is the number of values below the i-th
 *     distinct value, the running count of the host rule, so no counts are needed.  Rounding of a
 *     subtraction is monotone, so a boundary with p_{i+1} <= target is never taken and the walk may
 *     search for the first one whose successor is above the target.  At most max_bins - 1 are taken.)
 * Deduplication.  A candidate that is not above the candidate before it (neighbouring doubles,
 *     repeated inf) is dropped; the rest, in order, are the feature's edges: strictly increasing, at most
 *     CCDGPU_TRAIN_MAX_EDGES.
 * The result is a pure function of x and max_bins: it does not depend on the order of the rows, on
 * launch shapes or on how the features are grouped. */
/* The checks of a request (no device needed).  0, or CCDGPU_EINVAL with the reason in
 * ccdgpu_last_error(), naming the argument, and for a non-finite value its row and feature: a count
 * outside the limits above; with n_rows > 0, a NULL x or a non-finite x. */
int ccdgpu_splits_check(const double *x, int64_t n_rows, int32_t n_features, int32_t max_bins);
/* Check and find the edges: edges [n_features][CCDGPU_TRAIN_MAX_EDGES] gets feature f's edges at
 * edges[f][0 .. n_edges[f]) and zeros behind them, n_edges [n_features] their counts (what
 * ccdgpu_forest_train takes once packed back to back).  Synchronous; *kernel_seconds (may be NULL)
 * gets the device time of the kernels.  x goes up in the slabs training uses; the features are sorted
 * in groups whose two key buffers (16 bytes per row and feature) stay within 2 GiB, a single feature's
 * where n_rows alone exceeds that (CCDGPU_SPLITS_GROUP_FEATURES in the environment, a test knob, fixes
 * the group size); the result does not depend on the grouping.  The context's forest and the trained
 * forest are untouched.  Refused with CCDGPU_EINVAL while a detection begun with
 * ccdgpu_run_slot_begin is not finished. */
int ccdgpu_forest_find_splits(ccdgpu_ctx *ctx, const double *x, int64_t n_rows, int32_t n_features, int32_t max_bins,
                              double *edges, int32_t *n_edges, double *kernel_seconds);

/* Out-of-bag evaluation of a forest: every row scored only by the trees whose bag it is not in.
 * The bags are not stored: w(t,r) of the training rule above is a function of (seed, t, r), so
 * "row r is out of tree t's bag" is recomputed wherever it is needed.
 *
 * The rule.  For the context's forest (ccdgpu_forest_set), a seed, and row i of x with hash index
 * r = first_row + i:
 *     raw[:] = 0.0 (double); n = 0
 *     for t = 0 .. n_trees-1, in this order:
 *         u = H(seed, t, r, 0) >> 32
 *         if u >= P[0]: continue          (P = CCDGPU_TRAIN_POISSON; u < P[0]  <=>  w(t,r) == 0)
 *         walk tree t as ccdgpu_classify does; raw[:] += value[leaf][:]; n += 1
 *     oob_raw[i][:] = (float) raw[:]      (round to nearest);   n_oob[i] = n
 * Double adds in tree order and one float rounding, as rfrawp: only the tree set differs per row,
 * and a restatement in numpy is equal array by array.  A row with n_oob == 0 gets zeros, not NaN:
 * the count says it was not scored.  The rule holds for any checked forest and any seed, not only
 * for a trained forest and its own seed (with them, and first_row the row's index in the training
 * matrix, it is the out-of-bag estimate).  A NaN feature value goes right, as in the walk.
 * Limits: first_row >= 0, n_rows >= 0, first_row + n_rows <= CCDGPU_TRAIN_MAX_ROWS.  The result of
 * a row does not depend on how rows are batched: rows [a, b) with first_row = a are the slice of
 * the whole call. */
typedef struct ccdgpu_oob_params {
    uint64_t seed;              /* the training request's seed                              */
    int64_t first_row;          /* hash index of row 0 of x                                 */
} ccdgpu_oob_params;
#define CCDGPU_OOB_CUT 1580030168u /* CCDGPU_TRAIN_POISSON[0]: u below it is a weight of 0 */
/* The checks an out-of-bag request passes before anything reaches the device (no device needed).
 * 0, or CCDGPU_EINVAL with the reason in ccdgpu_last_error(), naming the argument: params NULL; a
 * count outside the limits above; with n_rows > 0, a NULL array.  x is not scanned: the walk
 * defines what a NaN does. */
int ccdgpu_oob_check(const double *x, int64_t n_rows, const ccdgpu_oob_params *params, const float *oob_raw,
                     const int32_t *n_oob);
/* x [n_rows][n_features] -> oob_raw [n_rows][n_classes], n_oob [n_rows] by the rule above, in slabs
 * of rows like ccdgpu_classify.  Synchronous; *kernel_seconds (may be NULL) gets the device time of
 * the kernel.  n_rows == 0 succeeds without a launch; CCDGPU_EINVAL with no forest set, and while a
 * detection begun with ccdgpu_run_slot_begin is not finished.  The context's forest, the trained
 * forest and the last run are untouched. */
int ccdgpu_forest_oob(ccdgpu_ctx *ctx, const double *x, int64_t n_rows, const ccdgpu_oob_params *params, float *oob_raw,
                      int32_t *n_oob, double *kernel_seconds);
/* The trained forest's weighted class counts, the c_k of the training rule: counts
 * [n_nodes][n_classes] in the node order of ccdgpu_trained_fetch (value[k] = c_k / n there).
 * CCDGPU_EINVAL when nothing has been trained, or when cap < n_nodes * n_classes. */
int ccdgpu_trained_counts(ccdgpu_ctx *ctx, int64_t *counts, int64_t cap);

/* Out-of-bag permutation importances of a forest (Breiman; R randomForest's MeanDecreaseAccuracy):
 * per tree, how many of the rows out of its bag it votes right, and how many of those votes are lost
 * or gained when one feature's column is shuffled.  Every output is an integer count.
 *
 * The rule.  For the context's forest (ccdgpu_forest_set), x [n_rows][n_features] (the whole training
 * matrix in training order: row i has hash index i, and the donors below come from all of it), labels
 * [n_rows] in 0 .. n_classes-1, a training seed and a perm_seed, with n = n_rows:
 *   vote(t, v): walk tree t over the feature vector v as ccdgpu_classify does (a NaN goes right); at
 *       the leaf, the lowest k with the largest value[leaf][k] (doubles compared as they are).
 *   out of bag: H(seed, t, r, 0) >> 32 < CCDGPU_OOB_CUT, the test of ccdgpu_forest_oob.
 *   the permutation of column f for tree t, a bijection of 0 .. n-1:
 *       k  = H(perm_seed, t, f, 2^32)      (the last argument is beyond every value training uses)
 *       b  = (k >> 32) mod n;   a0 = (k & 0xffffffff) mod n
 *       a  = the first of a0, a0+1, .. (wrapping from n-1 to 0) with gcd(a, n) == 1
 *       donor(t, f, r) = (a*r + b) mod n   (uint64; the product stays below 2^55)
 *     n == 1 gives a = 0 and donor 0.  The column is permuted over all rows, not only those out of
 *     the bag; only the rows out of the bag are evaluated.
 *   for every tree t and every row r out of t's bag, with y = labels[r]:
 *       oob_rows[t][y] += 1
 *       base = vote(t, x[r]) == y;   correct[t][y] += base
 *       for every feature f:  xp = x[r] with xp[f] = x[donor(t, f, r)][f];  perm = vote(t, xp) == y
 *           lost[t][f][y]   += base && !perm
 *           gained[t][f][y] += !base && perm
 * Votes and comparisons are exact, so the counts depend on no launch shape and no order of addition,
 * and a restatement in numpy is equal array by array.  (A feature a row's path does not test cannot
 * change its vote: only those on the path are re-walked.)
 * Limits: 1 <= n_rows <= CCDGPU_TRAIN_MAX_ROWS, so that every count is at most 2^27; n_rows == 0
 * succeeds with all-zero outputs. */
typedef struct ccdgpu_permutation_params {
    uint64_t seed;              /* the training request's seed: which rows are out of which bag */
    uint64_t perm_seed;         /* the seed of the columns' permutations                        */
} ccdgpu_permutation_params;
#define CCDGPU_PERM_HASH_C 4294967296ull /* 2^32, the last argument of H for a permutation's key */
/* The checks a permutation request passes before anything reaches the device (no device needed).
 * 0, or CCDGPU_EINVAL with the reason in ccdgpu_last_error() ("permutation: ..."), naming the
 * argument: params or an output NULL; n_rows, n_features or n_classes outside the limits; with
 * n_rows > 0, x or labels NULL, or a label outside 0 .. n_classes-1 (with its index).  x is not
 * scanned: the walk defines what a NaN does. */
int ccdgpu_permutation_check(const double *x, const int32_t *labels, int64_t n_rows, int32_t n_features, int32_t n_classes,
                             const ccdgpu_permutation_params *params, const int64_t *oob_rows, const int64_t *correct,
                             const int64_t *lost, const int64_t *gained);
/* The counts of the rule above: oob_rows and correct [n_trees][n_classes], lost and gained
 * [n_trees][n_features][n_classes], zeroed by every call.  x is held whole on the device for the call
 * (CCDGPU_ENOMEM when it does not fit).  Synchronous; *kernel_seconds (may be NULL) gets the device
 * time of the kernel.  CCDGPU_EINVAL with no forest set, and while a detection begun with
 * ccdgpu_run_slot_begin is not finished.  The context's forest, the trained forest and the last run
 * are untouched. */
int ccdgpu_forest_permutation(ccdgpu_ctx *ctx, const double *x, const int32_t *labels, int64_t n_rows,
                              const ccdgpu_permutation_params *params, int64_t *oob_rows, int64_t *correct, int64_t *lost,
                              int64_t *gained, double *kernel_seconds);

/* Prediction of band values from segment models: the modelled surface reflectance of every pixel
 * at dates of the caller's choosing (pyccd's ccd.models.lasso.predict over coefficient_matrix;
 * annual composites, synthetic images, residuals of observations against their model).
 *
 * The rule.  A pixel's rows are ccdgpu_row records in table order; `dates` [n_dates] are proleptic
 * ordinals shared by the pixels of the call, in any order, repeats allowed.
 *   basis of a date t:   w = 2 pi / avg_days_yr;  w12 = w * (double)t;  w34 = 2.0 * w12;
 *                        w56 = 3.0 * w12;  B = [t, cos w12, sin w12, cos w34, sin w34, cos w56,
 *                        sin w56]   (the lines of the detection's own basis)
 *   the row t takes:     rows with has_model == 0 (pyccd.default's row) are never taken;
 *                        CCDGPU_COVER_SPAN    the first row in table order with sday <= t <= eday;
 *                        CCDGPU_COVER_EXTEND  the row with the greatest sday <= t, ties going to the
 *                                             later row (the model holds through the gap after a
 *                                             break and after the last segment);
 *                        no such row: the fill
 *   value of band b:     v = intercept[b];  v = v + coef[b][k] * B[k] for k = 0 .. 6 in this order --
 *                        double arithmetic on the row's float32 values widened, every product and
 *                        every sum rounded on its own (no fused multiply-add)
 *   CCDGPU_PREDICT_F32:  (float)v rounded to nearest; a NaN v and the fill are the quiet NaN
 *                        0x7fc00000
 *   CCDGPU_PREDICT_I16:  rint(v) (halves to even) clamped to [-32768, 32767]; a NaN v and the fill
 *                        are -9999, the ARD fill value
 * A restatement of these lines in numpy, given the same basis (ccdgpu_coefficient_matrix), is
 * bit-equal; a value does not depend on how pixels or dates are batched or launched.
 *   out        [7][n_pix][n_dates] float or int16: band-major, date-contiguous, dates in the order
 *              given -- the layout of the `spectra` input, so a prediction at a chip's own dates
 *              subtracts from its observations directly
 *   seg_index  [n_pix][n_dates] int32, may be NULL: the taken row's index within its pixel, or -1 */
enum { CCDGPU_COVER_SPAN = 0, CCDGPU_COVER_EXTEND = 1 };
enum { CCDGPU_PREDICT_F32 = 0, CCDGPU_PREDICT_I16 = 1 };
#define CCDGPU_PREDICT_MAX_DATE 3652059 /* date.max.toordinal() */
/* The checks a prediction's arguments pass before anything reaches the device (no device needed).
 * 0, or CCDGPU_EINVAL with the reason in ccdgpu_last_error(): a NULL array; a negative count;
 * row_offsets[0] != 0, decreasing offsets, row_offsets[n_pix] != n_rows; a date outside
 * 1 .. CCDGPU_PREDICT_MAX_DATE (or more than 2^31 - 1 dates); a non-finite or non-positive
 * avg_days_yr; an unknown cover or dtype.  rows may be NULL when n_rows is 0, dates when n_dates is. */
int ccdgpu_predict_check(int64_t n_pix, const int64_t *row_offsets, int64_t n_rows, const ccdgpu_row *rows,
                         int64_t n_dates, const int64_t *dates, double avg_days_yr, int32_t cover, int32_t dtype);
/* Host-table path: pixel p has rows[row_offsets[p] .. row_offsets[p + 1]).  Runs the check first
 * (n_rows = row_offsets[n_pix]); synchronous; *kernel_seconds (may be NULL) gets the device time of
 * the kernels.  n_pix == 0 or n_dates == 0 succeeds without a launch.  The output is produced on the
 * device in slabs of whole pixels, so device memory stays bounded for any table.  Refused with
 * CCDGPU_EINVAL while a detection begun with ccdgpu_run_slot_begin is not finished. */
int ccdgpu_predict(ccdgpu_ctx *ctx, int64_t n_pix, const int64_t *row_offsets, const ccdgpu_row *rows, int64_t n_dates,
                   const int64_t *dates, double avg_days_yr, int32_t cover, int32_t dtype, void *out, int32_t *seg_index,
                   double *kernel_seconds);
/* Chained path: the same for the pixels of chip `chip` of the context's last completed run, from
 * its segments on the device -- each value narrowed to float32 exactly as the row packer does, so
 * the output equals ccdgpu_predict's on the rows ccdgpu_fetch_rows gives for that chip.  A pixel
 * without segments has no model.  Preconditions as ccdgpu_classify_rows (it works after
 * ccdgpu_run_slot_end_rows too); a chip index out of range is CCDGPU_EINVAL. */
int ccdgpu_predict_rows(ccdgpu_ctx *ctx, int32_t chip, int64_t n_dates, const int64_t *dates, double avg_days_yr,
                        int32_t cover, int32_t dtype, void *out, int32_t *seg_index, double *kernel_seconds);
/* The device's basis of `dates`: basis [n_dates][7], the B of the rule above -- the reference's
 * coefficient_matrix(dates, avg_days_yr, 8) -- which is what makes exact tests of the rule possible. */
int ccdgpu_coefficient_matrix(ccdgpu_ctx *ctx, int64_t n_dates, const int64_t *dates, double avg_days_yr, double *basis);

/* Annual change and land-cover product rasters from segments: per pixel and product date (LCMAP's
 * are the 1 July of each year) the time of spectral change, the change magnitude, the time since the
 * last change, the spectral stability period, the model quality, the primary and secondary land
 * cover with their confidences and the annual land-cover change.  The reference ecosystem's product
 * generator (lcmap-gaia) is not pinned here, so parity with it is not claimed: the rule below is
 * normative, and where gaia's choice is not certain it is a parameter (bot, mag_bands, cover, labels).
 *
 * The rule.  A pixel's rows are ccdgpu_row records in table order; `dates` [n_dates] are proleptic
 * ordinals shared by the pixels of the call, in any order, repeats allowed.  For a date t, a(t) is the
 * ordinal of 1 January of t's proleptic-Gregorian calendar year and b(t) that of the next 1 January
 * (ccdgpu_year_window; integer arithmetic on the host).  A row is a MODEL iff has_model != 0; it is a
 * BREAK iff it is a model, chprob == 1.0f and bday >= 1.  Day comparisons are on integers.
 * Change products, per pixel and date index i with date t:
 *   sctime  uint16  the first break in table order with a(t) <= bday < b(t): bday - a(t) + 1 (the day
 *                   of the year, 1 .. 366); no such break: 0
 *   scmag   float   of that same row: s = 0.0; for band b = 0 .. 6 with bit b of mag_bands set, in this
 *                   order, m = (double)mag[b], s = s + m * m (the product and the sum each rounded on
 *                   its own); the value is (float)sqrt(s), sqrt correctly rounded and the narrowing
 *                   to nearest; a NaN result is the quiet NaN 0x7fc00000; no such row: 0.0f
 *   sclast  uint16  min(t - g, 65535), g the greatest bday over breaks with bday <= t; no such break: 0
 *   scstab  uint16  min(t - g, 65535), g the greatest value over all models of sday (when sday <= t)
 *                   and, for breaks, bday (when bday <= t); none: min(t - bot, 65535) if t >= bot,
 *                   else 0
 *   scmqa   uint8   curqa, clamped to 0 .. 255, of the first model in table order with
 *                   sday <= t <= eday; none: 0
 * Cover products need rfrawp [n_rows][n_classes] float, row-aligned with the rows, n_classes >= 1:
 *   the row r of (pixel, t) is the one the prediction's rule takes under `cover` (CCDGPU_COVER_SPAN /
 *   CCDGPU_COVER_EXTEND).  The cover products are UNDEFINED when there is no such row, when any of
 *   rfrawp[r][0 .. n_classes) is NaN, or when S -- the sum of the values widened to double, in class
 *   order, each add rounded -- is not a finite value above 0.  Otherwise i1 is the index of the
 *   largest value, ties going to the lowest index, and i2 the same with i1 excluded (none when
 *   n_classes == 1).
 *   lcpri   uint8   labels[i1]; undefined: 0
 *   lcsec   uint8   labels[i2]; undefined or no i2: 0
 *   lcpconf uint8   rint(100.0 * (double)rfrawp[r][i1] / S) clamped to 0 .. 100 (the product and the
 *                   quotient each rounded on its own, halves to even); undefined: 0
 *   lcsconf uint8   the same with i2; undefined or no i2: 0
 *   lcachg  uint16  date index 0: 0; i > 0: with c = lcpri at date index i and q = lcpri at date index
 *                   i - 1, in the order the dates were given, q * 256 + c when both are non-zero and
 *                   differ, else 0 (whether or not lcpri itself is requested)
 * Every product is an array [n_dates][n_pix]: date-major, pixel-contiguous, each date one raster plane
 * in pixel order (a 100 x 100 chip's plane is its raster).  A NULL pointer in struct ccdgpu_products: that
 * product is not wanted.  A value does not depend on how pixels are batched, slabbed or launched; a
 * restatement of these lines in numpy is bit-equal. */
typedef struct ccdgpu_product_params {
    int64_t bot;                /* 723546   the beginning of time, 1982-01-01 (scstab)            */
    uint32_t mag_bands;         /* 0x3E     bit mask, green .. swir2: the detection bands (scmag) */
    int32_t cover;              /* CCDGPU_COVER_EXTEND                                            */
    int32_t n_classes;          /* 0 .. 32; 0: no cover products                                  */
    uint8_t labels[32];         /* k + 1    product value of class k, 1 .. 255                    */
    int32_t reserved0;          /* 0                                                              */
} ccdgpu_product_params;
void ccdgpu_product_params_default(ccdgpu_product_params *p);
/* the ten outputs (no typedef: the tag shares its name with the function below) */
struct ccdgpu_products {
    uint16_t *sctime;
    float *scmag;
    uint16_t *sclast, *scstab;
    uint8_t *scmqa;
    uint8_t *lcpri, *lcsec, *lcpconf, *lcsconf;
    uint16_t *lcachg;
};
/* a(t) and b(t) of the rule for t in 1 .. CCDGPU_PREDICT_MAX_DATE (else CCDGPU_EINVAL); host only. */
int ccdgpu_year_window(int64_t t, int64_t *a, int64_t *b);
/* The checks a product request passes before anything reaches the device (no device needed): every
 * check ccdgpu_predict_check makes on counts, offsets and dates, and CCDGPU_EINVAL with the reason
 * for: params or out NULL; bot outside 1 .. CCDGPU_PREDICT_MAX_DATE; mag_bands with bits above 6;
 * n_classes outside 0 .. 32; a label of 0 among the first n_classes; an unknown cover; a cover output
 * requested with rfrawp == NULL or n_classes == 0; all ten outputs NULL. */
int ccdgpu_products_check(int64_t n_pix, const int64_t *row_offsets, int64_t n_rows, const ccdgpu_row *rows,
                          const float *rfrawp, int64_t n_dates, const int64_t *dates, const ccdgpu_product_params *params,
                          const struct ccdgpu_products *out);
/* Host-table path: pixel p has rows[row_offsets[p] .. row_offsets[p + 1]) and, with rfrawp, their
 * rfrawp rows.  Runs the check first (n_rows = row_offsets[n_pix]); synchronous; *kernel_seconds (may
 * be NULL) gets the device time of the kernels.  n_pix == 0 or n_dates == 0 succeeds without a launch.
 * The output is produced on the device in slabs of whole pixels (at most 256 MiB of device output, or
 * CCDGPU_PRODUCT_SLAB_PIXELS pixels from the environment, a test knob), each requested product of a
 * slab copied back with one strided copy.  Refused with CCDGPU_EINVAL while a detection begun with
 * ccdgpu_run_slot_begin is not finished. */
int ccdgpu_products(ccdgpu_ctx *ctx, int64_t n_pix, const int64_t *row_offsets, const ccdgpu_row *rows, const float *rfrawp,
                    int64_t n_dates, const int64_t *dates, const ccdgpu_product_params *params,
                    const struct ccdgpu_products *out, double *kernel_seconds);
/* Chained path: the same for the pixels of chip `chip` of the context's last completed run, from its
 * segments on the device -- magnitude and change_probability narrowed to float32 exactly as the row
 * packer does, every segment a model -- so the output equals ccdgpu_products' on the rows
 * ccdgpu_fetch_rows gives for that chip.  rfrawp (may be NULL) holds that chip's rows in
 * ccdgpu_fetch_rows / ccdgpu_classify_rows order, pyccd.default's row of a pixel without segments
 * included.  Preconditions and error codes as ccdgpu_predict_rows. */
int ccdgpu_products_rows(ccdgpu_ctx *ctx, int32_t chip, const float *rfrawp, int64_t n_dates, const int64_t *dates,
                         const ccdgpu_product_params *params, const struct ccdgpu_products *out, double *kernel_seconds);
/* The number of rows ccdgpu_fetch_rows gives for chip `chip` of the last completed run -- what the
 * rfrawp of ccdgpu_products_rows must hold, and where the chip's rows lie among the batch's of
 * ccdgpu_classify_rows (chips in order) -- from the host's copy of the segment offsets: no device work. */
int ccdgpu_chip_row_count(ccdgpu_ctx *ctx, int32_t chip, int64_t *n_rows);

/* Kernel statistics of the last run (per launch of the main detection kernel). */
typedef struct ccdgpu_stats {
    double detect_ms;           /* average duration of the detection kernel (HIP events)   */
    double prep_ms;             /* average duration of the per-chip preparation kernel     */
    int64_t pixels;             /* pixels processed by the last run                        */
    int64_t segments;           /* segments written                                        */
    int64_t lasso_fits;         /* band-model fits (7 per model)                           */
    int64_t cd_sweeps;          /* coordinate-descent sweeps summed over fits              */
    int64_t flops;              /* counted FP64 flops (SURVEY.md §8(d) op-count model)     */
    int64_t bytes;              /* algorithmic HBM bytes read+written                      */
    double detect_ms_device;    /* the detection kernel's execution window, first wave in to
                                   last wave out, on the device's 100 MHz clock (excludes time
                                   queued behind another context's launch)                 */
    int64_t pool_reruns;        /* launches rerun because the segment pool overflowed      */
    int64_t pool_cap;           /* segment-pool capacity after the run (segments)          */
    int64_t wave_slots;         /* persistent detection waves of the launch (resident slots) */
    int64_t n_cu;               /* compute units the detection kernel may use              */
} ccdgpu_stats;
int ccdgpu_last_stats(ccdgpu_ctx *ctx, ccdgpu_stats *stats);

/* Raw device counters of the last run (up to 48 words): [0] band fits, [1] CD sweeps, [2] counted
 * flops, [8 + k] phase-k cycle totals (only in the diagnostic build lib/libccdgpu_diag.so). */
int ccdgpu_diag_counters(ccdgpu_ctx *ctx, uint64_t *out, int32_t n);

#ifdef __cplusplus
}
#endif
#endif
