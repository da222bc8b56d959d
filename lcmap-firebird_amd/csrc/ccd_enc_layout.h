/* ccd_enc_layout.h -- the byte layout of a transport-encoded batch, defined once for the host
 * encoder (ccd_encode.c), the host check (encoded_check in ccdgpu_checks.cpp) and the device readers
 * (ccd_decode_enc / ccd_decode_pack in ccd_pack.hip, px_setup in ccd_kernels.hip).
 *
 * The normative description is the comment above ccdgpu_encode_chips in include/ccdgpu.h; the
 * assertions below pin this file to the byte offsets documented there.  Plain C99 that also
 * compiles as HIP host and device code.  Everything here is a constant, a field, or a pure
 * function of a chip's shape (and, for mode 2, of the header's code_words): a locator reads no
 * memory, so a reader decides itself which header fields it loads, and when.
 *
 *   batch:   chip table | section 0 | section 1 | ...          (each 256-aligned)
 *   section: header (128 B) | parts of its mode, each 16-aligned
 *     mode 0: raw QA | raw spectra
 *     mode 1: kept offsets | 4-bit QA code rows | band columns
 *     mode 2: kept offsets | 4-bit QA code rows | run table | codes + pad word | exceptions
 * A locator takes the section's first byte and returns the part's, stepping from the part before
 * it; the section sizes add up the same part sizes.  The forms are chosen so that the device
 * readers compile to the instructions they had with the offsets written out by hand (compare
 * lib/ccd_kernels.s and a listing of ccd_pack.hip before and after a change here): n_obs stays
 * 32-bit through (n_obs + 1) / 2 and is widened afterwards, and parts are reached as
 * (sec + header) + bytes, not sec + (header + bytes). */
#ifndef CCD_ENC_LAYOUT_H
#define CCD_ENC_LAYOUT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define CCD_ENC_FN __host__ __device__ __forceinline__
#else
#define CCD_ENC_FN static inline
#endif
#ifdef __cplusplus
#define CCD_ENC_ASSERT(c, m) static_assert(c, m)
#else
#define CCD_ENC_ASSERT(c, m) _Static_assert(c, m)
#endif

enum {
    CCD_ENC_HDR = 128,   /* bytes of a section header */
    CCD_ENC_ALIGN = 256, /* alignment of the sections (and of the chip table's size) */
    CCD_ENC_BANDS = 7,
    CCD_ENC_MODE_RAW = 0,   /* the chip as it is */
    CCD_ENC_MODE_COLS = 1,  /* palette codes + compacted int16 band columns */
    CCD_ENC_MODE_PACK = 2   /* palette codes + bit-packed band runs */
};

typedef struct {
    int32_t mode, n_pix, n_obs, n_pal;
    uint16_t pal[16];
    int64_t kept, data_off, band_stride, pix_base;
    uint32_t drop_bits, pad0;
    int64_t code_words, exc_total; /* mode 2 only */
    uint8_t reserved[24];
} ccd_enc_hdr;
CCD_ENC_ASSERT(sizeof(ccd_enc_hdr) == CCD_ENC_HDR, "section header size");
CCD_ENC_ASSERT(offsetof(ccd_enc_hdr, pal) == 16, "palette");
CCD_ENC_ASSERT(offsetof(ccd_enc_hdr, kept) == 48 && offsetof(ccd_enc_hdr, data_off) == 56 &&
                   offsetof(ccd_enc_hdr, band_stride) == 64 && offsetof(ccd_enc_hdr, pix_base) == 72,
               "int64 block");
CCD_ENC_ASSERT(offsetof(ccd_enc_hdr, drop_bits) == 80, "drop_bits");
CCD_ENC_ASSERT(offsetof(ccd_enc_hdr, code_words) == 88 && offsetof(ccd_enc_hdr, exc_total) == 96, "mode 2 totals");

/* mode 2: the descriptor of one (pixel, band) run; run[n_pix][CCD_ENC_BANDS] */
typedef struct {
    int16_t base;
    uint16_t w;
    uint32_t code_word, exc_off, n_exc;
} ccd_enc_run;
CCD_ENC_ASSERT(sizeof(ccd_enc_run) == 16, "run descriptor size");

CCD_ENC_FN int64_t ccd_enc_up16(int64_t x) { return (x + 15) & ~(int64_t)15; }
CCD_ENC_FN int64_t ccd_enc_up_align(int64_t x) { return (x + CCD_ENC_ALIGN - 1) & ~(int64_t)(CCD_ENC_ALIGN - 1); }

/* ---- chip table: int64 n_chips; int64 chip_off[n_chips + 1]; int64 chip_pix[n_chips + 1] */
CCD_ENC_FN int64_t ccd_enc_n_chips(const uint8_t *enc) { return ((const int64_t *)enc)[0]; }
CCD_ENC_FN const int64_t *ccd_enc_chip_off(const uint8_t *enc) { return (const int64_t *)enc + 1; }
CCD_ENC_FN const int64_t *ccd_enc_chip_pix(const uint8_t *enc, int64_t n_chips) {
    return (const int64_t *)enc + 2 + n_chips;
}
CCD_ENC_FN int64_t ccd_enc_table_used(int64_t n_chips) { return 8 + 16 * (n_chips + 1); }
CCD_ENC_FN int64_t ccd_enc_table_bytes(int64_t n_chips) { return ccd_enc_up_align(ccd_enc_table_used(n_chips)); }
/* Declares int64_t lo = the chip that holds batch pixel pix: the last c with chip_pix[c] <= pix.
 * A statement macro, not a function: an inlined device function is optimised once on its own and
 * again in the kernel, and the decode kernels then differ from the hand-written loop (in the
 * operand order of one add) -- with the macro they are the same instruction for instruction. */
#define CCD_ENC_FIND_CHIP(lo, chip_pix, n_chips, pix) \
    int64_t lo = 0;                                   \
    for (int64_t hi_ = (n_chips)-1; lo < hi_;) {      \
        const int64_t mid_ = (lo + hi_ + 1) >> 1;     \
        if ((chip_pix)[mid_] <= (pix)) lo = mid_;     \
        else hi_ = mid_ - 1;                          \
    }

/* ---- parts of a section: the bytes of each (padded to 16), then where it starts */
CCD_ENC_FN int64_t ccd_enc_row_bytes(int32_t n_obs) { return (n_obs + 1) / 2; } /* one pixel's 4-bit code row */
CCD_ENC_FN int64_t ccd_enc_band_stride(int64_t kept) { return (kept + 7) & ~(int64_t)7; }
CCD_ENC_FN int64_t ccd_enc_raw_qa_bytes(int64_t plane) { return ccd_enc_up16(2 * plane); } /* plane = n_pix * n_obs */
CCD_ENC_FN int64_t ccd_enc_koff_bytes(int64_t n_pix) { return ccd_enc_up16(4 * (n_pix + 1)); }
CCD_ENC_FN int64_t ccd_enc_q4_bytes(int64_t n_pix, int32_t n_obs) {
    return ccd_enc_up16(n_pix * ccd_enc_row_bytes(n_obs));
}
CCD_ENC_FN int64_t ccd_enc_runs_bytes(int64_t n_pix) { return CCD_ENC_BANDS * (int64_t)sizeof(ccd_enc_run) * n_pix; }
CCD_ENC_FN int64_t ccd_enc_codes_bytes(int64_t code_words) { return ccd_enc_up16(4 * (code_words + 1)); } /* + pad word */
/* mode 0 */
CCD_ENC_FN const uint8_t *ccd_enc_raw_qa(const uint8_t *sec) { return sec + CCD_ENC_HDR; }
CCD_ENC_FN const uint8_t *ccd_enc_raw_spectra(const uint8_t *sec, int64_t plane) {
    return ccd_enc_raw_qa(sec) + ccd_enc_raw_qa_bytes(plane);
}
/* modes 1 and 2 */
CCD_ENC_FN const uint8_t *ccd_enc_koff(const uint8_t *sec) { return sec + CCD_ENC_HDR; }
CCD_ENC_FN const uint8_t *ccd_enc_q4(const uint8_t *sec, int64_t n_pix) {
    return ccd_enc_koff(sec) + ccd_enc_koff_bytes(n_pix);
}
/* behind the code rows: mode 1's band columns, mode 2's run table */
CCD_ENC_FN const uint8_t *ccd_enc_body(const uint8_t *sec, int64_t n_pix, int32_t n_obs) {
    return ccd_enc_q4(sec, n_pix) + ccd_enc_q4_bytes(n_pix, n_obs);
}
/* mode 2 */
CCD_ENC_FN const uint8_t *ccd_enc_codes(const uint8_t *sec, int64_t n_pix, int32_t n_obs) {
    return ccd_enc_body(sec, n_pix, n_obs) + ccd_enc_runs_bytes(n_pix);
}
CCD_ENC_FN const uint8_t *ccd_enc_exc(const uint8_t *sec, int64_t n_pix, int32_t n_obs, int64_t code_words) {
    return ccd_enc_codes(sec, n_pix, n_obs) + ccd_enc_codes_bytes(code_words);
}

/* ---- exact bytes of a section (before its padding to CCD_ENC_ALIGN): the header and its parts */
CCD_ENC_FN int64_t ccd_enc_size_raw(int64_t plane) {
    return CCD_ENC_HDR + ccd_enc_raw_qa_bytes(plane) + CCD_ENC_BANDS * 2 * plane;
}
CCD_ENC_FN int64_t ccd_enc_size_cols(int64_t n_pix, int32_t n_obs, int64_t band_stride) {
    return CCD_ENC_HDR + ccd_enc_koff_bytes(n_pix) + ccd_enc_q4_bytes(n_pix, n_obs) + CCD_ENC_BANDS * 2 * band_stride;
}
/* mode 2: up to the codes (what the shape alone fixes), and all of it */
CCD_ENC_FN int64_t ccd_enc_size_pack_fixed(int64_t n_pix, int32_t n_obs) {
    return CCD_ENC_HDR + ccd_enc_koff_bytes(n_pix) + ccd_enc_q4_bytes(n_pix, n_obs) + ccd_enc_runs_bytes(n_pix);
}
CCD_ENC_FN int64_t ccd_enc_size_pack(int64_t n_pix, int32_t n_obs, int64_t code_words, int64_t exc_total) {
    return ccd_enc_size_pack_fixed(n_pix, n_obs) + ccd_enc_codes_bytes(code_words) + 2 * exc_total;
}
/* most bytes of a chip section in mode 2.  A run of k values at width w holds ceil(k w / 32) code
 * words and e(w) exceptions: 4 ceil(k w / 32) + 2 e < (k w + 16 e) / 8 + 4 <= 2 k + 4, because the
 * canonical w minimises k w + 16 e(w) and w = 16 costs 16 k.  So the codes and exceptions of a chip
 * stay below mode 1's band columns + 4 bytes per run; added to mode 1's size: the run table, the
 * pad word, and the alignment of the codes and exceptions parts. */
CCD_ENC_FN int64_t ccd_enc_size_pack_bound(int64_t n_pix, int32_t n_obs) {
    return ccd_enc_size_cols(n_pix, n_obs, ccd_enc_band_stride(n_pix * n_obs)) + ccd_enc_runs_bytes(n_pix) +
           4 * CCD_ENC_BANDS * n_pix + 4 + 32;
}

#endif
