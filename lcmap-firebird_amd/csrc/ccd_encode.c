/* ccd_encode.c -- transport encoding of ARD chips for the PCIe upload (host side).
 *
 * The tile path is bound by the host-to-device link (16 bytes per observation: 7 int16 bands +
 * a uint16 QA word).  The encoding sends less of it:
 *   - the band values of an observation whose QA word has any of `drop_bits` set are not sent;
 *     the device writes -9999 (the ARD fill value) in their place.  With drop_bits = the fill bit
 *     (and strict_bits = the same: such an observation must hold -9999 in every band, or its chip
 *     goes raw) the encoding is lossless.  With the fill, cloud and shadow bits it drops values
 *     the detection never reads: pyccd's procedures (qa.standard_procedure_filter and the snow
 *     and insufficient-clear filters) keep only clear / water (/ snow) observations -- the class
 *     qabitval gives a word, fill > cloud > shadow > snow > water > clear -- so a word with the
 *     fill, cloud or shadow bit is never in a processing mask and its band values never enter a
 *     test or a fit (px_setup in ccd_kernels.hip: keep = class clear or water (or snow) and the
 *     range tests), and the results are the same (tests/test_gpu_encode.py, test_gpu_tile.py);
 *   - a chip's QA words take a handful of distinct values: each becomes a 4-bit index into a
 *     16-entry palette (a chip with more distinct words is sent raw, mode 0).
 * The device decoder (ccd_decode_enc in ccd_pack.hip) rebuilds the standard band-major
 * [7][n_pix][n_obs] spectra and [n_pix][n_obs] QA of every chip (tests/test_encode.py: round
 * trips against a numpy decoder).  Layout: described in include/ccdgpu.h, defined (offsets, part
 * locators, section sizes) in ccd_enc_layout.h.
 *   - with CCDGPU_ENC_PACK (ccdgpu_encode_chips_flags) the kept band values of each (pixel, band)
 *     travel as a base, a bit width and bit-packed residuals with an exception list (mode 2,
 *     decoded by ccd_decode_pack; tests/test_encode_pack.py) instead of as int16 columns.
 *
 * The encode replaces the copy into pinned memory that every upload from a fetched (pageable)
 * chip needs anyway; it runs one pass over the QA words (counts, palette, fill check) and one
 * over the bands (stream compaction: AVX-512 VBMI2 compress-store where the CPU has it).
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "ccd_enc_layout.h"
#include "ccdgpu.h"
#ifdef _OPENMP
#include <omp.h>
#endif

int64_t ccdgpu_encoded_bound_flags(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs, uint32_t flags) {
    if (n_chips <= 0 || !n_pix || !n_obs || (flags & ~CCDGPU_ENC_PACK)) return -1;
    int64_t t = ccd_enc_table_bytes(n_chips);
    for (int32_t c = 0; c < n_chips; ++c) {
        const int64_t plane = (int64_t)n_pix[c] * n_obs[c];
        const int64_t a = ccd_enc_size_raw(plane);
        const int64_t b = (flags & CCDGPU_ENC_PACK)
                              ? ccd_enc_size_pack_bound(n_pix[c], n_obs[c])
                              : ccd_enc_size_cols(n_pix[c], n_obs[c], ccd_enc_band_stride(plane));
        t += ccd_enc_up_align(a > b ? a : b);
    }
    return t;
}
int64_t ccdgpu_encoded_bound(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs) {
    return ccdgpu_encoded_bound_flags(n_chips, n_pix, n_obs, 0);
}

/* ---- band compaction: dst[k++] = src[i] for the observations kept (keep[i] = 1); *bad is set
 * when a dropped observation that must hold the fill value (strict[i] = 1) holds another one
 * (the chip then goes raw).  Only kept values are written: dst has room for exactly this pixel's
 * kept run, and the next pixel's run (another thread's, under the static schedule) follows it. */
static size_t compact_scalar(const int16_t *src, const uint8_t *keep, const uint8_t *strict, int n, int16_t *dst,
                             int *bad) {
    size_t k = 0;
    int b = 0;
    for (int i = 0; i < n; ++i) {
        if (keep[i]) dst[k++] = src[i];
        b |= strict[i] & (src[i] != -9999);
    }
    *bad |= b;
    return k;
}

#if defined(__x86_64__)
#include <immintrin.h>
/* Streaming writer of one contiguous output range (a block's run of one band): the compressed
 * values are staged in a small L1-resident buffer laid out like the destination lines, and every
 * destination line that lies wholly inside the range leaves with a non-temporal store -- no
 * read-for-ownership of the pinned destination, which costs a DRAM read of every line written
 * (the encoded batch, ~15 KB per tile pixel, is far larger than the caches).  The range's first
 * and last lines, which it may share with a neighbouring range (another block, possibly another
 * thread's), are written with masked ordinary stores of its own elements only. */
#define NTW_LINES 32
typedef struct {
    int16_t stage[(NTW_LINES + 1) * 32] __attribute__((aligned(64)));
    int16_t *dst; /* destination line of stage[0] (64-byte aligned) */
    int first;    /* elements of the range's first line below its start (0 once that line is out) */
    int k;        /* elements staged, counted from stage[0] */
} ntw_t;

__attribute__((target("avx512f,avx512bw"))) static inline void ntw_begin(ntw_t *w, int16_t *dst) {
    const uintptr_t a = (uintptr_t)dst;
    w->dst = (int16_t *)(a & ~(uintptr_t)63);
    w->first = (int)((a & 63) >> 1);
    w->k = w->first;
}
/* CCDGPU_ENCODE_NT=0: ordinary stores for the full lines too (A/B) */
static int ntw_stream(void) {
    static int v = -1;
    if (v < 0) {
        const char *e = getenv("CCDGPU_ENCODE_NT");
        v = !(e && *e == '0');
    }
    return v;
}
__attribute__((target("avx512f,avx512bw"))) static inline void ntw_lines(ntw_t *w, int nl) {
    const int nt = ntw_stream();
    for (int i = 0; i < nl; ++i) {
        const __m512i v = _mm512_load_si512((const void *)(w->stage + 32 * i));
        if (w->first) {
            _mm512_mask_storeu_epi16(w->dst, (__mmask32)(0xFFFFFFFFu << w->first), v);
            w->first = 0;
        } else if (nt) {
            _mm512_stream_si512((__m512i *)w->dst, v);
        } else {
            _mm512_store_si512((void *)w->dst, v);
        }
        w->dst += 32;
    }
}
/* c compressed values (the low lanes of v) onto the range */
__attribute__((target("avx512f,avx512bw"))) static inline void ntw_put(ntw_t *w, __m512i v, int c) {
    _mm512_mask_storeu_epi16(w->stage + w->k, (__mmask32)(c == 32 ? 0xFFFFFFFFu : (1u << c) - 1u), v);
    w->k += c;
    if (w->k >= NTW_LINES * 32) {
        const int nl = w->k >> 5;
        ntw_lines(w, nl);
        _mm512_store_si512((void *)w->stage, _mm512_load_si512((const void *)(w->stage + 32 * nl)));
        w->k -= 32 * nl;
    }
}
/* the range is complete: its full lines, then its partial last line */
__attribute__((target("avx512f,avx512bw"))) static inline void ntw_end(ntw_t *w) {
    const int nl = w->k >> 5;
    ntw_lines(w, nl);
    const int rem = w->k - 32 * nl;
    if (rem > 0) {
        const __m512i v = _mm512_load_si512((const void *)(w->stage + 32 * nl));
        _mm512_mask_storeu_epi16(w->dst, (__mmask32)(((1u << rem) - 1u) & (0xFFFFFFFFu << w->first)), v);
    }
    w->first = 0;
    w->k = 0;
}

/* the same with AVX-512 VBMI2, 32 observations at a time; m[] = keep bit masks, sm[] = the strict
 * observations' bit masks.  The kept values are compressed in a register and appended to the
 * range's streaming writer (a compress with a memory destination is microcoded and slow on Zen
 * 4/5). */
__attribute__((target("avx512f,avx512bw,avx512vbmi2"))) static size_t compact_vbmi2(const int16_t *src,
                                                                                   const uint32_t *m,
                                                                                   const uint32_t *sm, int n,
                                                                                   ntw_t *out, int *bad) {
    size_t k = 0;
    int i = 0, w = 0;
    const __m512i fillv = _mm512_set1_epi16(-9999);
    __mmask32 nb = 0;  /* dropped observations whose value is not the fill value */
    for (; i + 32 <= n; i += 32, ++w) {
        const __m512i v = _mm512_loadu_si512((const void *)(src + i));
        const int c = __builtin_popcount(m[w]);
        ntw_put(out, _mm512_maskz_compress_epi16((__mmask32)m[w], v), c);
        k += (size_t)c;
        nb |= _mm512_mask_cmpneq_epi16_mask((__mmask32)sm[w], v, fillv);
    }
    if (i < n) {
        const __mmask32 tail = (__mmask32)((1ull << (n - i)) - 1ull);
        const __m512i v = _mm512_maskz_loadu_epi16(tail, (const void *)(src + i));
        const int c = __builtin_popcount(m[w] & tail);
        ntw_put(out, _mm512_maskz_compress_epi16((__mmask32)(m[w] & tail), v), c);
        k += (size_t)c;
        nb |= _mm512_mask_cmpneq_epi16_mask((__mmask32)(sm[w] & tail), v, fillv);
    }
    *bad |= nb != 0;
    return k;
}
/* the same into a plain buffer (the packed encoder's staging row; dst holds n + 32 values: every
 * step stores a whole register at the run's end) */
__attribute__((target("avx512f,avx512bw,avx512vbmi2"))) static size_t compact_vbmi2_buf(const int16_t *src,
                                                                                       const uint32_t *m,
                                                                                       const uint32_t *sm, int n,
                                                                                       int16_t *dst, int *bad) {
    size_t k = 0;
    int i = 0, w = 0;
    const __m512i fillv = _mm512_set1_epi16(-9999);
    __mmask32 nb = 0;
    for (; i < n; i += 32, ++w) {
        const __mmask32 lm = n - i >= 32 ? (__mmask32)0xFFFFFFFFu : (__mmask32)((1u << (n - i)) - 1u);
        const __m512i v = _mm512_maskz_loadu_epi16(lm, (const void *)(src + i));
        _mm512_storeu_si512((void *)(dst + k), _mm512_maskz_compress_epi16((__mmask32)(m[w] & lm), v));
        k += (size_t)__builtin_popcount(m[w] & lm);
        nb |= _mm512_mask_cmpneq_epi16_mask((__mmask32)(sm[w] & lm), v, fillv);
    }
    *bad |= nb != 0;
    return k;
}
/* 4-bit palette codes (two per byte, even observation in the low nibble) and the keep bit masks
 * of one pixel's QA row, 32 observations at a time: a code is the index of the palette entry its
 * word equals (at most 16 compares); the codes' 16-bit lanes, read as 32-bit pairs, fold into
 * bytes with one down-convert.  Returns nonzero if a word is not in the palette (it got code 0
 * without being pal[0]): the palette came from a sample of the chip's pixels and misses it. */
__attribute__((target("avx512f,avx512bw,avx512vl,avx512vbmi2"))) static int qa_codes_avx512(const uint16_t *q, int n,
                                                                                  const uint16_t *pal, int npal,
                                                                                  uint16_t drop, uint16_t strict,
                                                                                  uint8_t *r, uint32_t *km,
                                                                                  uint32_t *sm) {
    int i = 0, w = 0;
    const __m512i dropv = _mm512_set1_epi16((short)drop), strictv = _mm512_set1_epi16((short)strict);
    const __m512i pal0 = _mm512_set1_epi16((short)pal[0]);
    __mmask32 miss = 0;
    for (; i < n; i += 32, ++w) {
        const __mmask32 lm = n - i >= 32 ? (__mmask32)0xFFFFFFFFu : (__mmask32)((1u << (n - i)) - 1u);
        const __m512i v = _mm512_maskz_loadu_epi16(lm, (const void *)(q + i));
        __m512i code = _mm512_setzero_si512();
        for (int j = 1; j < npal; ++j)
            code = _mm512_mask_mov_epi16(code, _mm512_cmpeq_epi16_mask(v, _mm512_set1_epi16((short)pal[j])),
                                         _mm512_set1_epi16((short)j));
        miss |= _mm512_mask_cmpneq_epi16_mask(_mm512_cmpeq_epi16_mask(code, _mm512_setzero_si512()) & lm, v, pal0);
        km[w] = (uint32_t)(_mm512_testn_epi16_mask(v, dropv) & lm);
        sm[w] = (uint32_t)(_mm512_test_epi16_mask(v, strictv) & lm);
        const __m512i pr = _mm512_or_si512(_mm512_and_si512(code, _mm512_set1_epi32(0xF)),
                                           _mm512_and_si512(_mm512_srli_epi32(code, 12), _mm512_set1_epi32(0xF0)));
        const __m128i bytes = _mm512_cvtepi32_epi8(pr);
        const int nb = (n - i >= 32 ? 32 : n - i + 1) / 2;  /* bytes of this chunk's codes */
        _mm_mask_storeu_epi8(r + (i >> 1), (__mmask16)(nb == 16 ? 0xFFFFu : (1u << nb) - 1u), bytes);
    }
    return miss != 0;
}
/* pass 1 of a pixel's QA row outside the palette sample: the dropped count only */
__attribute__((target("avx512f,avx512bw,avx512vl"))) static uint32_t qa_count_avx512(const uint16_t *q, int n,
                                                                                   uint16_t drop) {
    uint32_t fill = 0;
    const __m512i dv = _mm512_set1_epi16((short)drop);
    int i = 0;
    for (; i + 32 <= n; i += 32)
        fill += (uint32_t)__builtin_popcount(_mm512_test_epi16_mask(_mm512_loadu_si512((const void *)(q + i)), dv));
    if (i < n) {
        const __mmask32 lm = (__mmask32)((1u << (n - i)) - 1u);
        fill += (uint32_t)__builtin_popcount(_mm512_test_epi16_mask(_mm512_maskz_loadu_epi16(lm, (const void *)(q + i)), dv) & lm);
    }
    return fill;
}
/* pass 1 of one pixel's QA row, vector path: dropped count, and every word not yet in the thread's
 * list s_pal (compared 32 at a time against the list; the rare new word is added) */
__attribute__((target("avx512f,avx512bw,avx512vl,avx512vbmi2"))) static uint32_t qa_scan_avx512(const uint16_t *q,
                                                                                               int n, uint16_t drop,
                                                                                               uint16_t *s_pal,
                                                                                               int *s_npal) {
    uint32_t fill = 0;
    const __m512i one = _mm512_set1_epi16((short)drop);
    int np = *s_npal;
    for (int i = 0; i < n; i += 32) {
        const __mmask32 lm = n - i >= 32 ? (__mmask32)0xFFFFFFFFu : (__mmask32)((1u << (n - i)) - 1u);
        const __m512i v = _mm512_maskz_loadu_epi16(lm, (const void *)(q + i));
        fill += (uint32_t)__builtin_popcount(_mm512_test_epi16_mask(v, one) & lm);
        __mmask32 hit = 0;  /* independent compares (an early-exit chain measured 1.7x slower) */
        for (int j = 0; j < np; ++j) hit |= _mm512_cmpeq_epi16_mask(v, _mm512_set1_epi16((short)s_pal[j]));
        __mmask32 un = lm & ~hit;
        while (un) {
            const uint16_t w = q[i + __builtin_ctz(un)];
            if (np < 17) s_pal[np++] = w;
            un &= ~_mm512_cmpeq_epi16_mask(v, _mm512_set1_epi16((short)w));
            if (np >= 17) un = 0;  /* more than a palette: the chip goes raw */
        }
    }
    *s_npal = np;
    return fill;
}
static int have_vbmi2(void) {
    static int v = -1;
    if (v < 0) {
        const char *e = getenv("CCDGPU_ENCODE_SCALAR");
        v = (e && *e && *e != '0') ? 0 : __builtin_cpu_supports("avx512vbmi2") && __builtin_cpu_supports("avx512bw") &&
                                                  __builtin_cpu_supports("avx512vl");
    }
    return v;
}
#else
static int have_vbmi2(void) { return 0; }
#endif

int32_t ccdgpu_encode_vector_path(void) { return have_vbmi2(); }

/* pixels per block of the vector pass 2 (CCDGPU_ENCODE_BLOCK overrides the default 32; 1 = the
 * bands of one pixel after another) */
static int enc_block(void) {
    static int b = 0;
    if (!b) {
        const char *e = getenv("CCDGPU_ENCODE_BLOCK");
        int v = e ? atoi(e) : 32;
        b = v < 1 ? 1 : v > 256 ? 256 : v;
    }
    return b;
}

/* per-thread pass-1 state: the QA words seen (a 65536-bit set), a fill observation with a band
 * value other than -9999 */
typedef struct {
    /* scalar path: byte flags (independent stores, no read-modify-write chain); 8-aligned in every
     * element of the per-thread array, for the merge that reads them as 64-bit words */
    uint8_t seen[65536] __attribute__((aligned(8)));
    uint16_t pal[17];     /* vector path: the distinct words met so far (17 = more than a palette holds) */
    int npal;
    int bad_fill;
} pass1_t;

/* mode 0: the chip as it is (header fields other than the mode already written) */
static size_t encode_raw(int32_t n_pix, int32_t n_obs, const int16_t *spectra, const uint16_t *qa, uint8_t *sec,
                         int nt) {
    const size_t plane = (size_t)n_pix * (size_t)n_obs;
    ccd_enc_hdr *h = (ccd_enc_hdr *)sec;
    h->mode = CCD_ENC_MODE_RAW;
    h->n_pal = 0;
    h->kept = 0;
    h->band_stride = 0;
    memset(h->pal, 0, sizeof h->pal);
    uint16_t *oq = (uint16_t *)ccd_enc_raw_qa(sec);
    int16_t *os = (int16_t *)ccd_enc_raw_spectra(sec, (int64_t)plane);
    memset(oq + plane, 0, (size_t)ccd_enc_raw_qa_bytes((int64_t)plane) - 2 * plane);
#pragma omp parallel for schedule(static) num_threads(nt)
    for (int32_t p = 0; p < n_pix; ++p) {
        memcpy(oq + (size_t)p * n_obs, qa + (size_t)p * n_obs, 2 * (size_t)n_obs);
        for (int b = 0; b < 7; ++b)
            memcpy(os + (size_t)b * plane + (size_t)p * n_obs, spectra + (size_t)b * plane + (size_t)p * n_obs,
                   2 * (size_t)n_obs);
    }
    return (size_t)ccd_enc_size_raw((int64_t)plane);
}

/* pixels of a chip whose QA rows pass 1 scans for the palette (vector path): every
 * ENC_SAMPLE-th; pass 2 checks every word against it and, when one is missing, the chip is
 * encoded again from a scan of every pixel.  The palette is the chip's sorted set of distinct
 * words either way, so the bytes are the same. */
#define ENC_SAMPLE 16

/* ---- mode 2: bit-packed band runs (layout and the canonical width in include/ccdgpu.h; the run
 * descriptor ccd_enc_run in ccd_enc_layout.h) */

/* one run: the kept values v[0..k) of a (pixel, band) -> its descriptor (code_word / exc_off left
 * to the caller), its code words at cw and its exceptions at ex; returns the code words written */
static uint32_t pk_pack_run(const int16_t *v, int k, ccd_enc_run *r, uint32_t *cw, int16_t *ex) {
    int mn = 0;
    if (k > 0) {
        mn = 32767;
        for (int i = 0; i < k; ++i) mn = v[i] < mn ? v[i] : mn;
    }
    /* hist[j] = values with bitlen(r + 1) = j (1 .. 17): e(w) = the count of r >= 2^w - 1, that is
     * of bitlen(r + 1) > w, is a suffix sum */
    uint32_t hist[18] = {0};
    for (int i = 0; i < k; ++i) hist[32 - __builtin_clz((uint32_t)(v[i] - mn) + 1u)]++;
    int w = 0;
    if (hist[1] != (uint32_t)k) {
        uint32_t best = 0xFFFFFFFFu;
        uint32_t suf[19];
        suf[18] = 0;
        for (int j = 17; j >= 1; --j) suf[j] = suf[j + 1] + hist[j];
        for (int c = 1; c <= 16; ++c) {  /* ascending, strictly better only: ties go to the smallest w */
            const uint32_t e = c < 16 ? suf[c + 1] : 0u;
            const uint32_t cost = (uint32_t)c * (uint32_t)k + 16u * e;
            if (cost < best) {
                best = cost;
                w = c;
            }
        }
    }
    r->base = (int16_t)mn;
    r->w = (uint16_t)w;
    uint32_t nw = 0, ne = 0;
    if (w > 0) {
        const uint32_t esc = w < 16 ? (1u << w) - 1u : 0xFFFFFFFFu;
        uint64_t acc = 0;
        int nb = 0;
        for (int i = 0; i < k; ++i) {
            uint32_t c = (uint32_t)(v[i] - mn);
            if (c >= esc) {
                c = esc;
                ex[ne++] = v[i];
            }
            acc |= (uint64_t)c << nb;
            nb += w;
            if (nb >= 32) {
                cw[nw++] = (uint32_t)acc;
                acc >>= 32;
                nb -= 32;
            }
        }
        if (nb > 0) cw[nw++] = (uint32_t)acc;
    }
    r->n_exc = ne;
    return nw;
}

#if defined(__x86_64__)
__attribute__((target("avx512f,avx512bw"))) static inline int pk_min16(__m512i v) {
    int16_t t[32] __attribute__((aligned(64)));
    _mm512_store_si512((void *)t, v);
    int m = t[0];
    for (int i = 1; i < 32; ++i) m = t[i] < m ? t[i] : m;
    return m;
}
__attribute__((target("avx512f,avx512bw"))) static inline unsigned pk_max16u(__m512i v) {
    uint16_t t[32] __attribute__((aligned(64)));
    _mm512_store_si512((void *)t, v);
    unsigned m = t[0];
    for (int i = 1; i < 32; ++i) m = t[i] > m ? t[i] : m;
    return m;
}
/* pk_pack_run with AVX-512 (VBMI2 compress for the exceptions) and BMI2 pext for the bit packing:
 * the same descriptor, words and exceptions (tests/test_encode_pack.py compares the bytes).  rb:
 * k + 64 values of scratch; cw and ex may be written up to 16 words / 32 values past the run (the
 * next run's place in the staging, or its slack).  The width search walks down from the narrowest
 * width without escapes, W = bitlen(max r + 1) (cost W k), and stops at the first w whose escapes
 * alone cost as much as the best so far: e(w) only grows below it, so nothing there can win or
 * tie; going down, `<=` hands a tie to the smaller w, as the canonical choice wants. */
__attribute__((target("avx512f,avx512bw,avx512vl,avx512vbmi2,bmi2"))) static uint32_t pk_pack_run_vec(
    const int16_t *v, int k, ccd_enc_run *r, uint32_t *cw, int16_t *ex, uint16_t *rb) {
    r->base = 0;
    r->w = 0;
    r->n_exc = 0;
    if (k <= 0) return 0;
    __m512i mnv = _mm512_set1_epi16(32767);
    for (int i = 0; i < k; i += 32) {
        const __mmask32 lm = k - i >= 32 ? (__mmask32)0xFFFFFFFFu : (__mmask32)((1u << (k - i)) - 1u);
        mnv = _mm512_min_epi16(mnv, _mm512_mask_loadu_epi16(mnv, lm, (const void *)(v + i)));
    }
    const int mn = pk_min16(mnv);
    r->base = (int16_t)mn;
    const __m512i bv = _mm512_set1_epi16((short)mn);
    __m512i mxv = _mm512_setzero_si512();
    for (int i = 0; i < k; i += 32) {  /* residuals (mod 2^16 = the unsigned difference); 0 past the run */
        const __mmask32 lm = k - i >= 32 ? (__mmask32)0xFFFFFFFFu : (__mmask32)((1u << (k - i)) - 1u);
        const __m512i rr = _mm512_maskz_sub_epi16(lm, _mm512_maskz_loadu_epi16(lm, (const void *)(v + i)), bv);
        _mm512_storeu_si512((void *)(rb + i), rr);
        mxv = _mm512_max_epu16(mxv, rr);
    }
    _mm512_storeu_si512((void *)(rb + (k + 31) / 32 * 32), _mm512_setzero_si512());
    const unsigned mx = pk_max16u(mxv);
    if (mx == 0) return 0;
    int W = 32 - __builtin_clz(mx + 1u);
    if (W > 16) W = 16;
    int w = W;
    uint32_t best = (uint32_t)W * (uint32_t)k;
    for (int c = W - 1; c >= 1; --c) {
        const __m512i thr = _mm512_set1_epi16((short)((1u << c) - 1u));
        uint32_t e = 0;
        for (int i = 0; i < k; i += 32)
            e += (uint32_t)__builtin_popcount(_mm512_cmpge_epu16_mask(_mm512_loadu_si512((const void *)(rb + i)), thr));
        const uint32_t cost = (uint32_t)c * (uint32_t)k + 16u * e;
        if (cost <= best) {
            best = cost;
            w = c;
        }
        if (16u * e >= best) break;
    }
    r->w = (uint16_t)w;
    uint32_t ne = 0;
    if (w < 16) {  /* codes in place of the residuals; the escapes' raw values to the exception list */
        const __m512i escv = _mm512_set1_epi16((short)((1u << w) - 1u));
        for (int i = 0; i < k; i += 32) {
            const __m512i rr = _mm512_loadu_si512((const void *)(rb + i));
            const __mmask32 m = _mm512_cmpge_epu16_mask(rr, escv);
            _mm512_storeu_si512((void *)(rb + i), _mm512_min_epu16(rr, escv));
            if (m) {
                const __mmask32 lm = k - i >= 32 ? (__mmask32)0xFFFFFFFFu : (__mmask32)((1u << (k - i)) - 1u);
                _mm512_storeu_si512((void *)(ex + ne),
                                    _mm512_maskz_compress_epi16(m, _mm512_maskz_loadu_epi16(lm, (const void *)(v + i))));
                ne += (uint32_t)__builtin_popcount(m);
            }
        }
    }
    r->n_exc = ne;
    /* four codes at a time: pext gathers their low w bits into 4 w contiguous bits.  32 codes are
     * exactly w words, so every chunk of 32 starts on a word with an empty accumulator: the chunks'
     * shift / or chains do not depend on each other and overlap in the core.  The last chunk's
     * codes past the run are 0 (rb is zero to the chunk's end); its words past the run's last one
     * are zeros in the staging's next place or slack. */
    const uint64_t pm = (uint64_t)((1u << w) - 1u) * 0x0001000100010001ull;
    for (int ch = 0; ch < (k + 31) / 32; ++ch) {
        const uint16_t *src = rb + 32 * ch;
        uint32_t *o = cw + (size_t)ch * (size_t)w;
        uint64_t acc = 0;
        int nb = 0;
#pragma GCC unroll 8
        for (int g = 0; g < 8; ++g) {
            uint64_t x;
            memcpy(&x, src + 4 * g, 8);
            x = _pext_u64(x, pm);
            const uint64_t hi = nb ? x >> (64 - nb) : 0;
            acc |= x << nb;
            nb += 4 * w;
            if (nb >= 64) {
                memcpy(o, &acc, 8);
                o += 2;
                acc = hi;
                nb -= 64;
            }
            if (nb >= 32) {
                *o++ = (uint32_t)acc;
                acc >>= 32;
                nb -= 32;
            }
        }
    }
    return ((uint32_t)k * (uint32_t)w + 31u) / 32u;
}
#endif

/* the scalar path's QA row: 4-bit codes, keep and strict flags per observation */
static void pk_qa_scalar(const uint16_t *q, int n, const uint8_t *lut, uint16_t drop, uint16_t strict, uint8_t *r,
                         uint8_t *keep, uint8_t *strictm) {
    for (int i = 0; i < n; ++i) {
        const uint16_t v = q[i];
        if (i & 1) r[i >> 1] |= (uint8_t)(lut[v] << 4);
        else r[i >> 1] = lut[v];
        keep[i] = (uint8_t)!(v & drop);
        strictm[i] = (uint8_t)((v & strict) != 0);
    }
}

/* a block's staged code words into the section: the streaming writer where the vector path runs
 * (full lines leave with non-temporal stores, the lines shared with the neighbouring blocks with
 * masked stores of the block's own words), memcpy otherwise */
#if defined(__x86_64__)
__attribute__((target("avx512f,avx512bw"))) static void pk_stream_out(uint32_t *dst, const uint32_t *src, size_t words) {
    ntw_t w;
    const int16_t *s = (const int16_t *)src;
    size_t n = 2 * words;
    ntw_begin(&w, (int16_t *)dst);
    for (; n >= 32; n -= 32, s += 32) ntw_put(&w, _mm512_loadu_si512((const void *)s), 32);
    if (n) ntw_put(&w, _mm512_maskz_loadu_epi16((__mmask32)((1u << n) - 1u), (const void *)s), (int)n);
    ntw_end(&w);
}
#endif

/* pass 2 of a packed chip: QA codes, the run table, code words and exceptions behind the header,
 * kept offsets and (already padded) code rows of `sec`.  Blocks of pixels are packed into
 * thread-local staging (each raw row is read once) and committed in block order -- the ordered
 * region hands out the block's first code word and exception -- so the prefix sums, and with them
 * the bytes, do not depend on the thread count.  Returns the section's bytes; 0 when memory ran
 * out; *miss / *bad as pass 2 of mode 1 reports them (the caller encodes again / sends raw);
 * *bad also when the totals leave 32 bits. */
static size_t pk_pass2(int32_t n_pix, int32_t n_obs, const int16_t *spectra, const uint16_t *qa, uint8_t *sec,
                       uint8_t *q4, size_t rowb, const uint16_t *pal, int npal, const uint8_t *lut, uint16_t drop,
                       uint16_t strict, int nt, int *miss_out, int *bad_out) {
    const size_t plane = (size_t)n_pix * (size_t)n_obs;
    ccd_enc_run *runs = (ccd_enc_run *)ccd_enc_body(sec, n_pix, n_obs);
    uint32_t *codes = (uint32_t *)ccd_enc_codes(sec, n_pix, n_obs);
    const int vec = have_vbmi2();
    const int pb = enc_block();
    const int mw = n_obs / 32 + 2;
    const size_t rw = (size_t)n_obs / 2 + 1;  /* most code words of a run (w = 16) */
    uint64_t g_cw = 0, g_ex = 0;              /* committed so far (ordered region only) */
    int16_t *gex = NULL;                      /* the chip's exceptions until their place is known */
    size_t gex_cap = 0;
    int oom = 0, bad2 = 0, miss = 0;
#pragma omp parallel num_threads(nt) reduction(| : bad2, miss)
    {
        int16_t *vals = (int16_t *)malloc(2 * ((size_t)n_obs + 64));
        uint8_t *keep = (uint8_t *)malloc(2 * (size_t)n_obs + 64), *strictm = keep ? keep + n_obs + 32 : NULL;
        uint32_t *km = (uint32_t *)malloc((size_t)mw * 8), *sm = km ? km + mw : NULL;
        uint32_t *cw = (uint32_t *)malloc(4 * ((size_t)pb * 7 * rw + 32));             /* (+ the vector packer's slack) */
        int16_t *ex = (int16_t *)malloc(2 * ((size_t)pb * 7 * (size_t)n_obs + 64));
        uint16_t *rb = (uint16_t *)malloc(2 * ((size_t)n_obs + 128));
        ccd_enc_run *rs = (ccd_enc_run *)malloc(sizeof(ccd_enc_run) * 7 * (size_t)pb);
        const int ok = vals && keep && km && cw && ex && rs && rb;
#pragma omp for schedule(static, 1) ordered
        for (int32_t p0 = 0; p0 < n_pix; p0 += pb) {
            const int32_t pe = p0 + pb < n_pix ? p0 + pb : n_pix;
            uint32_t bw = 0, be = 0;  /* the block's code words and exceptions */
            for (int32_t p = p0; ok && p < pe; ++p) {
                const uint16_t *q = qa + (size_t)p * n_obs;
#if defined(__x86_64__)
                if (vec) miss |= qa_codes_avx512(q, n_obs, pal, npal, drop, strict, q4 + (size_t)p * rowb, km, sm);
                else
#endif
                    pk_qa_scalar(q, n_obs, lut, drop, strict, q4 + (size_t)p * rowb, keep, strictm);
                for (int b = 0; b < 7; ++b) {
                    const int16_t *src = spectra + (size_t)b * plane + (size_t)p * n_obs;
                    ccd_enc_run *r = rs + 7 * (size_t)(p - p0) + b;
                    uint32_t nw;
#if defined(__x86_64__)
                    if (vec) {
                        const size_t k = compact_vbmi2_buf(src, km, sm, n_obs, vals, &bad2);
                        nw = pk_pack_run_vec(vals, (int)k, r, cw + bw, ex + be, rb);
                    } else
#endif
                    {
                        const size_t k = compact_scalar(src, keep, strictm, n_obs, vals, &bad2);
                        nw = pk_pack_run(vals, (int)k, r, cw + bw, ex + be);
                    }
                    r->code_word = bw;
                    r->exc_off = be;
                    bw += nw;
                    be += r->n_exc;
                }
            }
            uint64_t my_cw = 0, my_ex = 0;
#pragma omp ordered
            {
                my_cw = g_cw;
                my_ex = g_ex;
                g_cw += bw;
                g_ex += be;
                if (!ok) oom = 1;
                if (be && !oom) {
                    if (g_ex > gex_cap) {
                        const size_t cap = (size_t)g_ex * 2 + 4096;
                        int16_t *n = (int16_t *)realloc(gex, 2 * cap);
                        if (n) {
                            gex = n;
                            gex_cap = cap;
                        } else {
                            oom = 1;
                        }
                    }
                    if (!oom) memcpy(gex + my_ex, ex, 2 * (size_t)be);
                }
            }
            if (!ok || my_cw + bw > 0xFFFFFFF0ull || my_ex + be > 0xFFFFFFF0ull) {
                bad2 |= ok;  /* totals past 32 bits: the chip goes raw */
                continue;
            }
            for (size_t i = 0; i < 7 * (size_t)(pe - p0); ++i) {
                rs[i].code_word += (uint32_t)my_cw;
                rs[i].exc_off += (uint32_t)my_ex;
            }
            memcpy(runs + 7 * (size_t)p0, rs, sizeof(ccd_enc_run) * 7 * (size_t)(pe - p0));
#if defined(__x86_64__)
            if (vec && bw) pk_stream_out(codes + my_cw, cw, bw);
            else
#endif
                memcpy(codes + my_cw, cw, 4 * (size_t)bw);
        }
#if defined(__x86_64__)
        if (vec) _mm_sfence();
#endif
        free(vals);
        free(keep);
        free(km);
        free(cw);
        free(ex);
        free(rb);
        free(rs);
    }
    *miss_out = miss;
    *bad_out = bad2;
    if (oom) {
        free(gex);
        return 0;
    }
    if (miss || bad2) {
        free(gex);
        return 1;  /* (any nonzero value: the caller looks at the flags first) */
    }
    /* the pad word and the padding of the codes part, then the exceptions */
    memset(codes + g_cw, 0, (size_t)ccd_enc_codes_bytes((int64_t)g_cw) - 4 * (size_t)g_cw);
    if (g_ex) memcpy((int16_t *)ccd_enc_exc(sec, n_pix, n_obs, (int64_t)g_cw), gex, 2 * (size_t)g_ex);
    free(gex);
    ccd_enc_hdr *h = (ccd_enc_hdr *)sec;
    h->code_words = (int64_t)g_cw;
    h->exc_total = (int64_t)g_ex;
    return (size_t)ccd_enc_size_pack(n_pix, n_obs, (int64_t)g_cw, (int64_t)g_ex);
}

/* one chip into sec (room for the larger of its two modes); returns the section's bytes */
static size_t encode_chip(int32_t n_pix, int32_t n_obs, const int16_t *spectra, const uint16_t *qa, int64_t pix_base,
                          int64_t data_off, uint8_t *sec, int threads, uint32_t *kept_scratch, uint16_t drop,
                          uint16_t strict, uint32_t flags) {
    const size_t plane = (size_t)n_pix * (size_t)n_obs;
    int nt = threads > 0 ? threads : 1;
    if (nt > 64) nt = 64;
    pass1_t *st = (pass1_t *)malloc((size_t)nt * sizeof(pass1_t));
    uint8_t *lut = (uint8_t *)malloc(65536);  /* QA word -> palette index */
    if (!st || !lut) {
        free(st);
        free(lut);
        return 0;
    }
    const int vec1 = have_vbmi2();
    /* a packed chip of few observations can be larger than the raw chip (the run table is 112 bytes
     * per pixel): such a chip is known to be encodable -- its full palette, its strict observations
     * -- before pass 2 writes anything, so that a chip that goes raw after all never had bytes
     * written behind the raw section the call returns */
    const int pack_small =
        (flags & CCDGPU_ENC_PACK) && ccd_enc_size_pack_bound(n_pix, n_obs) > ccd_enc_size_raw((int64_t)plane);
    size_t ret = 0;
    for (int full = vec1 && !pack_small ? 0 : 1; full < 2; ++full) {
        const int sample = full ? 1 : ENC_SAMPLE;
        memset(st, 0, (size_t)nt * sizeof(pass1_t));
        /* pass 1: kept counts, distinct QA words (of the sampled pixels) */
#pragma omp parallel for schedule(static) num_threads(nt)
        for (int32_t p = 0; p < n_pix; ++p) {
#ifdef _OPENMP
            pass1_t *s = &st[omp_get_thread_num()];
#else
            pass1_t *s = &st[0];
#endif
            const uint16_t *q = qa + (size_t)p * n_obs;
            uint32_t fill = 0;
#if defined(__x86_64__)
            if (vec1) {
                fill = p % sample == 0 ? qa_scan_avx512(q, n_obs, drop, s->pal, &s->npal) : qa_count_avx512(q, n_obs, drop);
            } else
#endif
            {
                for (int32_t i = 0; i < n_obs; ++i) {
                    const uint16_t v = q[i];
                    s->seen[v] = 1;
                    fill += (v & drop) != 0;
                }
            }
            kept_scratch[p] = (uint32_t)n_obs - fill;
        }
        int bad = 0;  /* (pass 2 checks the fill observations' band values) */
        uint16_t palv[16];
        int npal = 0;
        for (int t = 0; t < nt; ++t) bad |= st[t].bad_fill;
        if (vec1)  /* the threads' word lists into the byte set the scalar path fills */
            for (int t = 0; t < nt; ++t)
                for (int j = 0; j < st[t].npal; ++j) st[t].seen[st[t].pal[j]] = 1;
        for (int t = 0; t < nt; ++t)
            if (st[t].npal > 16) bad = 1;  /* (vector path: one thread alone met more than 16 words) */
        {
            uint64_t *s0 = (uint64_t *)st[0].seen;
            for (int t = 1; t < nt; ++t) {
                const uint64_t *st_ = (const uint64_t *)st[t].seen;
                for (int w = 0; w < 8192; ++w) s0[w] |= st_[w];
            }
            for (int w = 0; w < 8192 && npal <= 16; ++w)  /* ascending: the palette is sorted */
                if (s0[w])
                    for (int j = 0; j < 8 && npal <= 16; ++j)
                        if (st[0].seen[8 * w + j]) {
                            if (npal < 16) palv[npal] = (uint16_t)(8 * w + j);
                            ++npal;
                        }
        }
        ccd_enc_hdr *h = (ccd_enc_hdr *)sec;
        memset(h, 0, sizeof *h);
        h->n_pix = n_pix;
        h->n_obs = n_obs;
        h->data_off = data_off;
        h->pix_base = pix_base;
        if (bad || npal > 16) {
            ret = encode_raw(n_pix, n_obs, spectra, qa, sec, nt);
            break;
        }
        h->mode = CCD_ENC_MODE_COLS;
        h->n_pal = npal;
        h->drop_bits = drop;  /* the decoder's keep test */
        uint16_t *pal = h->pal;
        for (int j = 0; j < npal; ++j) {
            pal[j] = palv[j];
            lut[palv[j]] = (uint8_t)j;
        }
        uint32_t *koff = (uint32_t *)ccd_enc_koff(sec);
        uint64_t tot = 0;
        for (int32_t p = 0; p < n_pix; ++p) {
            koff[p] = (uint32_t)tot;
            tot += kept_scratch[p];
        }
        koff[n_pix] = (uint32_t)tot;
        /* padding after the offsets and after the code rows: deterministic bytes */
        memset(koff + n_pix + 1, 0, (size_t)ccd_enc_koff_bytes(n_pix) - 4 * ((size_t)n_pix + 1));
        const size_t bstride = (size_t)ccd_enc_band_stride((int64_t)tot);
        h->kept = (int64_t)tot;
        h->band_stride = (int64_t)bstride;
        uint8_t *q4 = (uint8_t *)ccd_enc_q4(sec, n_pix);
        const size_t rowb = (size_t)ccd_enc_row_bytes(n_obs);
        int16_t *bands = (int16_t *)ccd_enc_body(sec, n_pix, n_obs);
        memset(q4 + (size_t)n_pix * rowb, 0, (size_t)ccd_enc_q4_bytes(n_pix, n_obs) - (size_t)n_pix * rowb);
        if (flags & CCDGPU_ENC_PACK) {  /* mode 2: the band runs bit-packed instead of the band columns */
            int pmiss = 0, pbad = 0;
            if (pack_small && strict) {
#pragma omp parallel for schedule(static) num_threads(nt) reduction(| : pbad)
                for (int32_t p = 0; p < n_pix; ++p)
                    for (int32_t i = 0; i < n_obs; ++i)
                        if (qa[(size_t)p * n_obs + i] & strict)
                            for (int b = 0; b < 7; ++b)
                                pbad |= spectra[(size_t)b * plane + (size_t)p * n_obs + i] != -9999;
                if (pbad) {
                    ret = encode_raw(n_pix, n_obs, spectra, qa, sec, nt);
                    break;
                }
            }
            h->mode = CCD_ENC_MODE_PACK;
            h->band_stride = 0;
            const size_t sz = pk_pass2(n_pix, n_obs, spectra, qa, sec, q4, rowb, pal, npal, lut, drop, strict, nt,
                                       &pmiss, &pbad);
            if (sz && pmiss && !full) continue;
            ret = sz && pbad ? encode_raw(n_pix, n_obs, spectra, qa, sec, nt) : sz;
            break;
        }
        const int vec = have_vbmi2();
        int bad2 = 0, miss = 0;
        /* pass 2: 4-bit QA codes and the kept band values (and the fill observations' values checked).
         * Vector path in blocks of enc_block() pixels: the block's keep / strict masks first, then one
         * band at a time over the whole block, so the loads and stores run as two long sequential
         * streams (band rows of consecutive pixels are contiguous in the input plane and in the
         * output) instead of seven of each interleaved per pixel. */
        const int mw = n_obs / 32 + 2;  /* mask words per pixel */
        const int pb = enc_block();
#pragma omp parallel num_threads(nt) reduction(| : bad2, miss)
        {
            uint8_t *keep = (uint8_t *)malloc(2 * (size_t)n_obs + 64), *strictm = keep + n_obs + 32;
            uint32_t *km = (uint32_t *)malloc((size_t)mw * 8 * pb), *sm = km + (size_t)mw * pb;
#if defined(__x86_64__)
            ntw_t ntw_s; /* (2 KB, 64-byte aligned, on the thread's stack) */
            ntw_t *ntw = &ntw_s;
            if (vec) {
#pragma omp for schedule(static)
                for (int32_t p0 = 0; p0 < n_pix; p0 += pb) {
                    const int32_t pe = p0 + pb < n_pix ? p0 + pb : n_pix;
                    for (int32_t p = p0; p < pe; ++p)
                        miss |= qa_codes_avx512(qa + (size_t)p * n_obs, n_obs, pal, npal, drop, strict, q4 + (size_t)p * rowb,
                                                km + (size_t)(p - p0) * mw, sm + (size_t)(p - p0) * mw);
                    if (miss) continue;  /* the chip is encoded again */
                    for (int b = 0; b < 7; ++b) {
                        const int16_t *src = spectra + (size_t)b * plane;
                        /* the block's run of band b is one contiguous range (koff[p0] .. koff[pe]) */
                        ntw_begin(ntw, bands + (size_t)b * bstride + koff[p0]);
                        for (int32_t p = p0; p < pe; ++p)
                            compact_vbmi2(src + (size_t)p * n_obs, km + (size_t)(p - p0) * mw, sm + (size_t)(p - p0) * mw,
                                          n_obs, ntw, &bad2);
                        ntw_end(ntw);
                    }
                }
            } else
#endif
#pragma omp for schedule(static)
            for (int32_t p = 0; p < n_pix; ++p) {
                const uint16_t *q = qa + (size_t)p * n_obs;
                uint8_t *r = q4 + (size_t)p * rowb;
                memset(km, 0, ((size_t)n_obs / 32 + 1) * 4);
                int32_t i = 0;
                for (; i + 1 < n_obs; i += 2) {
                    const uint16_t v0 = q[i], v1 = q[i + 1];
                    r[i >> 1] = (uint8_t)(lut[v0] | (lut[v1] << 4));
                    const uint32_t k0 = !(v0 & drop), k1 = !(v1 & drop);
                    keep[i] = (uint8_t)k0;
                    keep[i + 1] = (uint8_t)k1;
                    strictm[i] = (uint8_t)((v0 & strict) != 0);
                    strictm[i + 1] = (uint8_t)((v1 & strict) != 0);
                    km[i >> 5] |= (k0 | (k1 << 1)) << (i & 31);
                }
                if (i < n_obs) {
                    const uint16_t v0 = q[i];
                    r[i >> 1] = lut[v0];
                    const uint32_t k0 = !(v0 & drop);
                    keep[i] = (uint8_t)k0;
                    strictm[i] = (uint8_t)((v0 & strict) != 0);
                    km[i >> 5] |= k0 << (i & 31);
                }
                for (int b = 0; b < 7; ++b)
                    compact_scalar(spectra + (size_t)b * plane + (size_t)p * n_obs, keep, strictm, n_obs,
                                   bands + (size_t)b * bstride + koff[p], &bad2);
            }
#if defined(__x86_64__)
            if (vec) _mm_sfence();  /* the streamed lines are visible before the batch is uploaded */
#endif
            free(keep);
            free(km);
        }
        if (miss && !full) continue;  /* a word the sample missed: every pixel's words this time */
        if (bad2) {
            ret = encode_raw(n_pix, n_obs, spectra, qa, sec, nt);  /* a strict observation with data */
            break;
        }
        for (int b = 0; b < 7; ++b)  /* band padding: deterministic bytes */
            memset(bands + (size_t)b * bstride + tot, 0, 2 * (bstride - (size_t)tot));
        ret = (size_t)ccd_enc_size_cols(n_pix, n_obs, (int64_t)bstride);
        break;
    }
    free(st);
    free(lut);
    return ret;
}

int64_t ccdgpu_encode_chips(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs, const int16_t *const *spectra,
                            const uint16_t *const *qa, uint8_t *out, int64_t out_cap, int32_t threads,
                            uint16_t drop_bits, uint16_t strict_bits) {
    return ccdgpu_encode_chips_flags(n_chips, n_pix, n_obs, spectra, qa, out, out_cap, threads, drop_bits, strict_bits,
                                     0);
}

int64_t ccdgpu_encode_chips_flags(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs,
                                  const int16_t *const *spectra, const uint16_t *const *qa, uint8_t *out,
                                  int64_t out_cap, int32_t threads, uint16_t drop_bits, uint16_t strict_bits,
                                  uint32_t flags) {
    if (n_chips <= 0 || !n_pix || !n_obs || !spectra || !qa || !out || (flags & ~CCDGPU_ENC_PACK)) return -1;
    if ((strict_bits & ~drop_bits) != 0) return -1;  /* a strict observation is a dropped one */
    const int64_t need = ccdgpu_encoded_bound_flags(n_chips, n_pix, n_obs, flags);
    if (need < 0 || out_cap < need) return -2;
    *(int64_t *)out = n_chips;  /* the chip table: n_chips, chip_off, chip_pix */
    int64_t *off = (int64_t *)ccd_enc_chip_off(out), *pix = (int64_t *)ccd_enc_chip_pix(out, n_chips);
    int32_t maxp = 0;
    for (int32_t c = 0; c < n_chips; ++c) {
        if (n_pix[c] <= 0 || n_obs[c] <= 0 || !spectra[c] || !qa[c]) return -1;
        maxp = n_pix[c] > maxp ? n_pix[c] : maxp;
    }
    uint32_t *kept = (uint32_t *)malloc(4 * (size_t)maxp);
    if (!kept) return -3;
    size_t pos = (size_t)ccd_enc_table_bytes(n_chips);
    memset(out + ccd_enc_table_used(n_chips), 0, pos - (size_t)ccd_enc_table_used(n_chips));  /* table padding */
    int64_t pbase = 0, dbase = 0;
    for (int32_t c = 0; c < n_chips; ++c) {
        off[c] = (int64_t)pos;
        pix[c] = pbase;
        const size_t sz = encode_chip(n_pix[c], n_obs[c], spectra[c], qa[c], pbase, dbase, out + pos, threads, kept,
                                      drop_bits, strict_bits, flags);
        if (!sz) {
            free(kept);
            return -3;
        }
        const size_t szp = (size_t)ccd_enc_up_align((int64_t)sz);
        memset(out + pos + sz, 0, szp - sz);  /* section padding */
        pos += szp;
        pbase += n_pix[c];
        dbase += (int64_t)n_pix[c] * n_obs[c];
    }
    off[n_chips] = (int64_t)pos;
    pix[n_chips] = pbase;
    free(kept);
    return (int64_t)pos;
}
