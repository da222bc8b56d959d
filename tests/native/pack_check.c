/* CPU check of the packed transport encoding (lcmap-firebird_amd/csrc/ccd_encode.c, mode 2 of
 * include/ccdgpu.h): random small chips -- band runs of random spread, so every width from 0 to
 * 16 and runs with exceptions occur -- are encoded with ccdgpu_encode_chips_flags(CCDGPU_ENC_PACK)
 * at random thread counts into a buffer filled with a sentinel, decoded by the plain-C decoder
 * below (parts located through csrc/ccd_enc_layout.h, which the encoder source includes; the
 * bit-by-bit decode is its own), and compared with the inputs; every byte behind the returned
 * count must still hold the sentinel.  Built with -fsanitize=address,undefined and run by tests/test_encode_pack.py. */
#include "../../lcmap-firebird_amd/csrc/ccd_encode.c"

#include <stdio.h>

static unsigned rs = 1;
#define RND() (rs = rs * 1103515245u + 12345u, (rs >> 8))

/* one section into sp [7][n_pix][n_obs] and qa [n_pix][n_obs]; 0 on success */
static int decode_section(const uint8_t *sec, int16_t *sp, uint16_t *qa) {
    ccd_enc_hdr h;
    memcpy(&h, sec, sizeof h);
    const uint32_t drop = h.drop_bits;
    const int64_t n_pix = h.n_pix, n_obs = h.n_obs, plane = n_pix * n_obs;
    if (h.mode == CCD_ENC_MODE_RAW) {
        memcpy(qa, ccd_enc_raw_qa(sec), 2 * (size_t)plane);
        memcpy(sp, ccd_enc_raw_spectra(sec, plane), 14 * (size_t)plane);
        return 0;
    }
    if (h.mode != CCD_ENC_MODE_PACK || h.band_stride != 0) return 1;
    const uint16_t *pal = h.pal;
    const uint32_t *koff = (const uint32_t *)ccd_enc_koff(sec);
    const int64_t rowb = ccd_enc_row_bytes(h.n_obs);
    const uint8_t *q4 = ccd_enc_q4(sec, n_pix);
    const ccd_enc_run *runs = (const ccd_enc_run *)ccd_enc_body(sec, n_pix, h.n_obs);
    const uint32_t *codes = (const uint32_t *)ccd_enc_codes(sec, n_pix, h.n_obs);
    const int16_t *exc = (const int16_t *)ccd_enc_exc(sec, n_pix, h.n_obs, h.code_words);
    if (codes[h.code_words] != 0) return 2; /* the pad word */
    for (int64_t p = 0; p < n_pix; ++p) {
        const int64_t k = (int64_t)koff[p + 1] - koff[p];
        for (int64_t i = 0; i < n_obs; ++i) qa[p * n_obs + i] = pal[(q4[p * rowb + i / 2] >> (4 * (i & 1))) & 15];
        for (int b = 0; b < 7; ++b) {
            const ccd_enc_run *r = runs + 7 * p + b;
            if (r->w > 16 || r->n_exc > k) return 3;
            int64_t rank = 0, er = 0;
            for (int64_t i = 0; i < n_obs; ++i) {
                int16_t v = -9999;
                if (!(qa[p * n_obs + i] & drop) && rank < k) {
                    uint32_t c = 0;
                    for (unsigned j = 0; j < r->w; ++j) {
                        const uint64_t bit = (uint64_t)rank * r->w + j;
                        c |= ((codes[r->code_word + (bit >> 5)] >> (bit & 31)) & 1u) << j;
                    }
                    if (r->w >= 1 && r->w <= 15 && c == (1u << r->w) - 1u) {
                        if (er >= r->n_exc) return 4;
                        v = exc[r->exc_off + er++];
                    } else {
                        v = (int16_t)(uint16_t)((uint32_t)(int32_t)r->base + c);
                    }
                    ++rank;
                }
                sp[(b * n_pix + p) * n_obs + i] = v;
            }
            if (rank != k || er != r->n_exc) return 5;
        }
    }
    return 0;
}

static int run(unsigned seed) {
    rs = seed;
    const int32_t n_chips = 1 + (int32_t)(RND() % 3);
    int32_t n_pix[3], n_obs[3];
    int16_t *sp[3];
    uint16_t *qa[3];
    for (int c = 0; c < n_chips; ++c) {
        n_pix[c] = 1 + (int32_t)(RND() % 70);
        n_obs[c] = 1 + (int32_t)(RND() % 150);
        const size_t plane = (size_t)n_pix[c] * n_obs[c];
        sp[c] = (int16_t *)malloc(14 * plane);
        qa[c] = (uint16_t *)malloc(2 * plane);
        const int many = RND() % 16 == 0; /* now and then more than 16 QA words: a raw chip */
        for (size_t i = 0; i < plane; ++i) {
            const unsigned t = RND() % 10;
            qa[c][i] = (uint16_t)(many ? 2 * (RND() % 400) : t == 0 ? 1 : t == 1 ? 66 | 32 : t == 2 ? 68 : 66);
        }
        for (int b = 0; b < 7; ++b)
            for (int32_t p = 0; p < n_pix[c]; ++p) {
                const unsigned spread = RND() % 18; /* the run's values span about 2^spread */
                const int32_t lo = (int32_t)(RND() % 65536) - 32768;
                const unsigned far = RND() % 3 ? RND() % 12 : 0; /* share of far-out values, in 64ths */
                for (int32_t i = 0; i < n_obs[c]; ++i) {
                    int32_t v = lo + (int32_t)(spread >= 17 ? RND() % 65536 : spread ? RND() % (1u << spread) : 0);
                    if (RND() % 64 < far) v = (int32_t)(RND() % 65536) - 32768;
                    if (v > 32767) v = 32767;
                    if (v < -32768) v = -32768;
                    const size_t at = ((size_t)b * n_pix[c] + p) * n_obs[c] + i;
                    sp[c][at] = (qa[c][(size_t)p * n_obs[c] + i] & 1) && !many ? (int16_t)-9999 : (int16_t)v;
                }
            }
    }
    const uint16_t drop = RND() % 2 ? 1 : 1 | 32 | 8;
    const int threads = 1 + (int)(RND() % 5);
    const int64_t bound = ccdgpu_encoded_bound_flags(n_chips, n_pix, n_obs, CCDGPU_ENC_PACK);
    const int64_t cap = bound + 4096;
    uint8_t *out = (uint8_t *)aligned_alloc(64, (size_t)(cap + 63) / 64 * 64);
    memset(out, 0xA5, (size_t)cap);
    const int64_t n = ccdgpu_encode_chips_flags(n_chips, n_pix, n_obs, (const int16_t *const *)sp,
                                                (const uint16_t *const *)qa, out, bound, threads, drop, 1,
                                                CCDGPU_ENC_PACK);
    int bad = 0;
    if (n <= 0 || n > bound) {
        printf("seed %u: encode returned %lld (bound %lld)\n", seed, (long long)n, (long long)bound);
        bad = 1;
    }
    for (int64_t i = n; !bad && i < cap; ++i)
        if (out[i] != 0xA5) {
            printf("seed %u: byte %lld behind the %lld returned was written\n", seed, (long long)i, (long long)n);
            bad = 1;
        }
    for (int c = 0; !bad && c < n_chips; ++c) {
        const size_t plane = (size_t)n_pix[c] * n_obs[c];
        int16_t *ds = (int16_t *)malloc(14 * plane);
        uint16_t *dq = (uint16_t *)malloc(2 * plane);
        int64_t off;
        memcpy(&off, out + 8 + 8 * c, 8);
        const int rc = decode_section(out + off, ds, dq);
        if (rc) {
            printf("seed %u: chip %d does not decode (%d)\n", seed, c, rc);
            bad = 1;
        }
        for (size_t i = 0; !bad && i < plane; ++i) {
            if (dq[i] != qa[c][i]) bad = 1;
            for (int b = 0; b < 7; ++b) {
                const int16_t want = (qa[c][i] & drop) && out[off] != 0 ? (int16_t)-9999 : sp[c][b * plane + i];
                if (ds[b * plane + i] != want) bad = 1;
            }
            if (bad) printf("seed %u: chip %d element %zu differs\n", seed, c, i);
        }
        free(ds);
        free(dq);
    }
    for (int c = 0; c < n_chips; ++c) {
        free(sp[c]);
        free(qa[c]);
    }
    free(out);
    return bad;
}

int main(void) {
    for (unsigned seed = 1; seed <= 200; ++seed)
        if (run(seed)) return 1;
    printf("vector path %d\nok\n", (int)ccdgpu_encode_vector_path());
    return 0;
}
