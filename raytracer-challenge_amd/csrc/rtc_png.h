// rtc_png.h — the arithmetic of the compressed PNG writer (include/rtc.h), shared by its host statement (host_png.cpp) and
// the device encoder (rtc_png.hip) so the two cannot drift: the row filters and their cost, the hash, the match of one
// position, the lazy rule, the deflate symbol tables, the length-limited Huffman build (package-merge), the run-length
// coding of the code lengths, the block costs and the block header. Only the order of work differs between them (serial
// on the host; per row, per position and per segment on the device). Not part of the ABI.
#ifndef RTC_PNG_H
#define RTC_PNG_H

#include <stddef.h>
#include <stdint.h>

#include "rtc.h"

#if defined(__HIPCC__)
#define RTC_PHD __host__ __device__ inline
#else
#define RTC_PHD inline
#endif

enum {
    RTC_PNG_WINDOW = 32768,
    RTC_PNG_MAX_MATCH = 258,
    RTC_PNG_HASH_SIZE = 32768,
    RTC_PNG_NLIT = 286,  // literal/length symbols that can occur (0..285)
    RTC_PNG_NDIST = 30,
    RTC_PNG_NCL = 19,
    RTC_PNG_MAX_RLE = RTC_PNG_NLIT + RTC_PNG_NDIST,
    // bytes of one segment's deflate data at most: its stored form (5-byte header + payload) and the sync flush (5 bytes)
    RTC_PNG_SEG_BYTES_MAX = 5 + RTC_PNG_SEGMENT + 5,
    // the fixed bytes of a file: signature 8, IHDR 25, zlib header 2, Adler-32 4, IEND 12; and 12 per IDAT chunk
    RTC_PNG_FILE_FIXED = 8 + 25 + 2 + 4 + 12,
    RTC_PNG_CHUNK_OVERHEAD = 12,
};
enum { RTC_PNG_STORED = 0, RTC_PNG_FIXED = 1, RTC_PNG_DYNAMIC = 2 };

// ---- filters (ISO 15948 §9): a = left, b = up, c = up-left (0 where outside the image) ----
RTC_PHD uint32_t rtc_png_paeth(uint32_t a, uint32_t b, uint32_t c) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p,
              pc = p > (int)c ? p - (int)c : (int)c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
RTC_PHD uint32_t rtc_png_filter_byte(uint32_t type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    switch (type) {
    case 0: return x;
    case 1: return (x - a) & 255u;
    case 2: return (x - b) & 255u;
    case 3: return (x - ((a + b) >> 1)) & 255u;
    default: return (x - rtc_png_paeth(a, b, c)) & 255u;
    }
}
RTC_PHD uint32_t rtc_png_filter_cost(uint32_t v) { return v < 128u ? v : 256u - v; }

// ---- matches ----
RTC_PHD uint32_t rtc_png_hash(uint32_t b0, uint32_t b1, uint32_t b2) { return ((b0 << 10) ^ (b1 << 5) ^ b2) & 0x7fffu; }

// The match at p of the filtered stream s[0, n): candidates are the RTC_PNG_CHAIN nearest q < p with p - q <= 32768 and the
// same hash, reached through prev[] (prev[q] = q - the nearest earlier position of q's hash, 0 if none within the window);
// length = common prefix, capped at 258 and at `end` (the end of p's segment). Returns the longest length >= 3 (ties: the
// nearest), 0 if none; *dist its distance.
RTC_PHD uint32_t rtc_png_match(const uint8_t *s, size_t n, const uint16_t *prev, size_t p, size_t end, uint32_t *dist) {
    *dist = 0;
    if (p + 3 > n || end < p + 3) return 0;
    const uint32_t cap = (uint32_t)((end - p) < RTC_PNG_MAX_MATCH ? (end - p) : RTC_PNG_MAX_MATCH);
    uint32_t best = 0;
    size_t q = p;
    for (uint32_t k = 0; k < RTC_PNG_CHAIN; ++k) {
        const uint32_t d = prev[q];
        if (d == 0 || p - (q - d) > RTC_PNG_WINDOW) break;
        q -= d;
        uint32_t l = 0;
        while (l < cap && s[q + l] == s[p + l]) ++l;
        if (l >= 3 && l > best) {
            best = l;
            *dist = (uint32_t)(p - q);
            if (l == cap) break;
        }
    }
    if (best < 3) *dist = 0;
    return best < 3 ? 0 : best;
}

// zlib's one-step lazy rule: a position with a match emits it unless the next position's match is longer
RTC_PHD bool rtc_png_takes_match(uint32_t l_here, uint32_t l_next) { return l_here >= 3 && !(l_next > l_here); }

// ---- deflate symbols (RFC 1951 §3.2.5) ----
constexpr uint16_t kPngLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint16_t kPngDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                       4097, 6145, 8193, 12289, 16385, 24577};
constexpr uint8_t kPngClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
RTC_PHD uint32_t rtc_png_len_base(uint32_t code) { return kPngLenBase[code]; } // code 0..28 of symbols 257..285
RTC_PHD uint32_t rtc_png_len_extra(uint32_t code) { return (code < 8 || code == 28) ? 0u : (code - 4) / 4; }
RTC_PHD uint32_t rtc_png_dist_base(uint32_t code) { return kPngDistBase[code]; }
RTC_PHD uint32_t rtc_png_dist_extra(uint32_t code) { return code < 4 ? 0u : (code - 2) / 2; }
RTC_PHD uint32_t rtc_png_len_code(uint32_t len) { // 3..258 -> 0..28
    uint32_t c = 0;
    while (c < 28 && rtc_png_len_base(c + 1) <= len) ++c;
    return c;
}
RTC_PHD uint32_t rtc_png_dist_code(uint32_t dist) { // 1..32768 -> 0..29
    uint32_t c = 0;
    while (c < 29 && rtc_png_dist_base(c + 1) <= dist) ++c;
    return c;
}
RTC_PHD uint32_t rtc_png_fixed_lit_len(uint32_t sym) { return sym < 144 ? 8u : sym < 256 ? 9u : sym < 280 ? 7u : 8u; }
RTC_PHD uint32_t rtc_png_cl_order(uint32_t i) { return kPngClOrder[i]; }
RTC_PHD uint32_t rtc_png_reverse(uint32_t code, uint32_t len) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1u - i);
    return r;
}

// ---- Huffman code lengths: package-merge, limited to `maxbits` ----
// Workspace of the build (LDS on the device): the sorted symbols, two levels' weights, each level's leaf flags, and what
// rtc_png_canonical and rtc_png_plan keep on the side.
struct PngHuffWork {
    uint16_t order[RTC_PNG_NLIT];
    uint32_t wa[2 * RTC_PNG_NLIT], wb[2 * RTC_PNG_NLIT];
    uint64_t leaf[15 * ((2 * RTC_PNG_NLIT + 63) / 64)];
    uint32_t count[16], next[16], clf[RTC_PNG_NCL];
    uint8_t seq[RTC_PNG_MAX_RLE];
};

// Lengths of an optimal prefix code of the symbols with freq > 0, no length above maxbits. Symbols are sorted by
// (freq, symbol) ascending. Lists: the deepest level holds the leaves; each level above merges the leaves with the pairs of
// the level below, in order, a leaf first when weights tie, and keeps its first 2m - 2 items (m = symbols used). The top
// level's first 2m - 2 items are taken; at each level the leaves among the items taken get one bit more, and its packages
// take two items each of the level below. Fewer than two symbols used: the used one (if any) and then the lowest-numbered
// unused symbols get length 1 until two have it.
RTC_PHD void rtc_png_huff_lengths(const uint32_t *freq, uint32_t nsym, uint32_t maxbits, uint8_t *len, PngHuffWork *w) {
    uint32_t m = 0;
    for (uint32_t i = 0; i < nsym; ++i) {
        len[i] = 0;
        if (freq[i]) w->order[m++] = (uint16_t)i;
    }
    if (m < 2) {
        for (uint32_t i = 0; i < m; ++i) len[w->order[i]] = 1;
        for (uint32_t i = 0, have = m; i < nsym && have < 2; ++i)
            if (!len[i]) { len[i] = 1; ++have; }
        return;
    }
    for (uint32_t i = 1; i < m; ++i) { // insertion sort by (freq, symbol)
        const uint16_t v = w->order[i];
        uint32_t j = i;
        while (j > 0 && freq[w->order[j - 1]] > freq[v]) { w->order[j] = w->order[j - 1]; --j; }
        w->order[j] = v;
    }
    const uint32_t keep = 2 * m - 2, words = (keep + 63) / 64;
    uint32_t *cur = w->wa, *nxt = w->wb;
    uint32_t cur_n = m < keep ? m : keep;
    for (uint32_t i = 0; i < cur_n; ++i) cur[i] = freq[w->order[i]];
    for (uint32_t k = 0; k < words; ++k) w->leaf[(maxbits - 1) * words + k] = 0;
    for (uint32_t i = 0; i < cur_n; ++i) w->leaf[(maxbits - 1) * words + i / 64] |= 1ull << (i % 64);
    for (int lev = (int)maxbits - 2; lev >= 0; --lev) {
        uint64_t *flags = w->leaf + (uint32_t)lev * words;
        for (uint32_t k = 0; k < words; ++k) flags[k] = 0;
        const uint32_t np = cur_n / 2;
        uint32_t a = 0, b = 0, o = 0;
        while (o < keep && (a < m || b < np)) {
            const uint32_t lw = a < m ? freq[w->order[a]] : 0u, pw = b < np ? cur[2 * b] + cur[2 * b + 1] : 0u;
            if (a < m && (b >= np || lw <= pw)) {
                nxt[o] = lw;
                flags[o / 64] |= 1ull << (o % 64);
                ++a;
            } else {
                nxt[o] = pw;
                ++b;
            }
            ++o;
        }
        uint32_t *t = cur; cur = nxt; nxt = t;
        cur_n = o;
    }
    uint32_t take = keep;
    for (uint32_t lev = 0; lev < maxbits && take; ++lev) {
        const uint64_t *flags = w->leaf + lev * words;
        uint32_t leaves = 0;
        for (uint32_t i = 0; i < take; ++i) leaves += (uint32_t)((flags[i / 64] >> (i % 64)) & 1u);
        for (uint32_t i = 0; i < leaves; ++i) ++len[w->order[i]];
        take = 2 * (take - leaves);
    }
}

// Canonical codes (RFC 1951 §3.2.2), stored bit-reversed for the LSB-first stream
RTC_PHD void rtc_png_canonical(const uint8_t *len, uint32_t nsym, uint16_t *code, PngHuffWork *w) {
    uint32_t *count = w->count, *next = w->next;
    for (uint32_t b = 0; b < 16; ++b) count[b] = next[b] = 0;
    for (uint32_t i = 0; i < nsym; ++i) ++count[len[i]];
    count[0] = 0;
    uint32_t c = 0;
    for (uint32_t b = 1; b < 16; ++b) {
        c = (c + count[b - 1]) << 1;
        next[b] = c;
    }
    for (uint32_t i = 0; i < nsym; ++i)
        code[i] = len[i] ? (uint16_t)rtc_png_reverse(next[len[i]]++, len[i]) : (uint16_t)0;
}

// Run-length coding of the code lengths (RFC 1951 §3.2.7) of one sequence: HLIT literal/length lengths, then HDIST distance
// lengths; runs may cross from one to the other. At each value v with a run of r equal values: v = 0: 18 for min(r, 138)
// while r >= 11, then 17 for r if r >= 3, else r zeros; v != 0: v once, then 16 for min(r, 6) while r >= 3, then v for the
// rest. Entry = symbol | repeat count << 5.
RTC_PHD uint32_t rtc_png_rle(const uint8_t *seq, uint32_t count, uint16_t *out) {
    uint32_t k = 0, i = 0;
    while (i < count) {
        const uint32_t v = seq[i];
        uint32_t r = 1;
        while (i + r < count && seq[i + r] == v) ++r;
        i += r;
        if (v == 0) {
            while (r >= 11) { const uint32_t t = r < 138 ? r : 138; out[k++] = (uint16_t)(18 | (t << 5)); r -= t; }
            if (r >= 3) { out[k++] = (uint16_t)(17 | (r << 5)); r = 0; }
            while (r) { out[k++] = 0; --r; }
        } else {
            out[k++] = (uint16_t)v;
            --r;
            while (r >= 3) { const uint32_t t = r < 6 ? r : 6; out[k++] = (uint16_t)(16 | (t << 5)); r -= t; }
            while (r) { out[k++] = (uint16_t)v; --r; }
        }
    }
    return k;
}
RTC_PHD uint32_t rtc_png_cl_extra_bits(uint32_t sym) { return sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u; }
RTC_PHD uint32_t rtc_png_cl_extra_value(uint32_t sym, uint32_t rep) { return sym == 16 ? rep - 3 : sym == 17 ? rep - 3 : rep - 11; }

// One segment's block: chosen type, its codes and, for a dynamic block, the header's parts.
struct PngPlan {
    uint32_t type, hlit, hdist, hclen, nrle;
    uint64_t bits[3];           // exact bits of the block as stored, fixed, dynamic (no padding, no sync flush)
    uint8_t lit_len[288], dist_len[32], cl_len[19];
    uint16_t lit_code[288], dist_code[32], cl_code[19];
    uint16_t rle[RTC_PNG_MAX_RLE];
};

// Plan the block of a segment of `nbytes` filtered bytes whose tokens have these symbol counts (lit: 0..285, 256 counted
// once; dist: 0..29) and `extra` extra bits in all. Cheapest of stored, fixed, dynamic by exact bit count; ties go to
// stored, then fixed.
RTC_PHD void rtc_png_plan(const uint32_t *lit, const uint32_t *dist, uint64_t extra, uint32_t nbytes, PngPlan *pl, PngHuffWork *w) {
    pl->bits[RTC_PNG_STORED] = 40ull + 8ull * nbytes;
    uint64_t fixed = 3 + extra;
    for (uint32_t i = 0; i < RTC_PNG_NLIT; ++i) fixed += (uint64_t)lit[i] * rtc_png_fixed_lit_len(i);
    for (uint32_t i = 0; i < RTC_PNG_NDIST; ++i) fixed += 5ull * dist[i];
    pl->bits[RTC_PNG_FIXED] = fixed;
    rtc_png_huff_lengths(lit, RTC_PNG_NLIT, 15, pl->lit_len, w);
    rtc_png_huff_lengths(dist, RTC_PNG_NDIST, 15, pl->dist_len, w);
    uint32_t hlit = RTC_PNG_NLIT, hdist = RTC_PNG_NDIST;
    while (hlit > 257 && pl->lit_len[hlit - 1] == 0) --hlit;
    while (hdist > 1 && pl->dist_len[hdist - 1] == 0) --hdist;
    uint8_t *seq = w->seq;
    for (uint32_t i = 0; i < hlit; ++i) seq[i] = pl->lit_len[i];
    for (uint32_t i = 0; i < hdist; ++i) seq[hlit + i] = pl->dist_len[i];
    pl->nrle = rtc_png_rle(seq, hlit + hdist, pl->rle);
    uint32_t *clf = w->clf;
    for (uint32_t i = 0; i < RTC_PNG_NCL; ++i) clf[i] = 0;
    for (uint32_t i = 0; i < pl->nrle; ++i) ++clf[pl->rle[i] & 31u];
    rtc_png_huff_lengths(clf, RTC_PNG_NCL, 7, pl->cl_len, w);
    uint32_t hclen = 19;
    while (hclen > 4 && pl->cl_len[rtc_png_cl_order(hclen - 1)] == 0) --hclen;
    pl->hlit = hlit;
    pl->hdist = hdist;
    pl->hclen = hclen;
    uint64_t dyn = 3 + 14 + 3ull * hclen + extra;
    for (uint32_t i = 0; i < pl->nrle; ++i) dyn += pl->cl_len[pl->rle[i] & 31u] + rtc_png_cl_extra_bits(pl->rle[i] & 31u);
    for (uint32_t i = 0; i < RTC_PNG_NLIT; ++i) dyn += (uint64_t)lit[i] * pl->lit_len[i];
    for (uint32_t i = 0; i < RTC_PNG_NDIST; ++i) dyn += (uint64_t)dist[i] * pl->dist_len[i];
    pl->bits[RTC_PNG_DYNAMIC] = dyn;
    const uint64_t st = pl->bits[0];
    pl->type = (st <= fixed && st <= dyn) ? RTC_PNG_STORED : fixed <= dyn ? RTC_PNG_FIXED : RTC_PNG_DYNAMIC;
    if (pl->type == RTC_PNG_FIXED) {
        for (uint32_t i = 0; i < 288; ++i) pl->lit_len[i] = (uint8_t)rtc_png_fixed_lit_len(i);
        for (uint32_t i = 0; i < 32; ++i) pl->dist_len[i] = 5;
    } else {
        for (uint32_t i = RTC_PNG_NLIT; i < 288; ++i) pl->lit_len[i] = 0;
        for (uint32_t i = RTC_PNG_NDIST; i < 32; ++i) pl->dist_len[i] = 0;
    }
    rtc_png_canonical(pl->lit_len, 288, pl->lit_code, w);
    rtc_png_canonical(pl->dist_len, 32, pl->dist_code, w);
    rtc_png_canonical(pl->cl_len, RTC_PNG_NCL, pl->cl_code, w);
}

// The block header: BFINAL and BTYPE, and for a dynamic block HLIT, HDIST, HCLEN, the code-length code and the coded lengths;
// for a stored block also the padding to the byte and LEN / NLEN (the segment starts on a byte). put(value, nbits), LSB first.
template <class Put>
RTC_PHD void rtc_png_block_header(const PngPlan &pl, bool final, uint32_t nbytes, Put &put) {
    put((final ? 1u : 0u) | (pl.type << 1), 3);
    if (pl.type == RTC_PNG_STORED) {
        put(0, 5);
        put(nbytes & 0xffffu, 16);
        put(~nbytes & 0xffffu, 16);
    } else if (pl.type == RTC_PNG_DYNAMIC) {
        put(pl.hlit - 257, 5);
        put(pl.hdist - 1, 5);
        put(pl.hclen - 4, 4);
        for (uint32_t i = 0; i < pl.hclen; ++i) put(pl.cl_len[rtc_png_cl_order(i)], 3);
        for (uint32_t i = 0; i < pl.nrle; ++i) {
            const uint32_t sym = pl.rle[i] & 31u, rep = pl.rle[i] >> 5;
            put(pl.cl_code[sym], pl.cl_len[sym]);
            if (sym >= 16) put(rtc_png_cl_extra_value(sym, rep), rtc_png_cl_extra_bits(sym));
        }
    }
}

// The bits of one token of a fixed or dynamic block (<= 48): a literal (len 0) or a match (len, dist); *nbits its length.
RTC_PHD uint64_t rtc_png_token_code(const PngPlan &pl, uint32_t literal, uint32_t len, uint32_t dist, uint32_t *nbits) {
    if (len == 0) {
        *nbits = pl.lit_len[literal];
        return pl.lit_code[literal];
    }
    const uint32_t lc = rtc_png_len_code(len), dc = rtc_png_dist_code(dist);
    const uint32_t le = rtc_png_len_extra(lc), de = rtc_png_dist_extra(dc);
    uint64_t v = pl.lit_code[257 + lc];
    uint32_t n = pl.lit_len[257 + lc];
    v |= (uint64_t)(len - rtc_png_len_base(lc)) << n;
    n += le;
    v |= (uint64_t)pl.dist_code[dc] << n;
    n += pl.dist_len[dc];
    v |= (uint64_t)(dist - rtc_png_dist_base(dc)) << n;
    n += de;
    *nbits = n;
    return v;
}

// ---- checksums ----
RTC_PHD uint32_t rtc_png_crc_table(uint32_t n) {
    uint32_t c = n;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}
// a * b modulo the CRC-32 polynomial (reflected), and x^(8n) modulo it: crc(A B) = mult(x8n(|B|), crc(A)) ^ crc(B)
RTC_PHD uint32_t rtc_png_crc_mult(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
RTC_PHD uint32_t rtc_png_crc_x8n(uint64_t n) {
    uint32_t p = 1u << 31, sq = 1u << 30; // x^0; x^1
    for (int k = 0; k < 3; ++k) sq = rtc_png_crc_mult(sq, sq); // x^8
    while (n) {
        if (n & 1u) p = rtc_png_crc_mult(sq, p);
        sq = rtc_png_crc_mult(sq, sq);
        n >>= 1;
    }
    return p;
}
RTC_PHD uint32_t rtc_png_crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    return rtc_png_crc_mult(rtc_png_crc_x8n(len_b), crc_a) ^ crc_b;
}

RTC_PHD void rtc_png_be32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}
// signature + IHDR without its CRC (the first 29 bytes); the caller adds the CRC of bytes 12..28
RTC_PHD void rtc_png_head(uint32_t width, uint32_t height, uint32_t channels, uint8_t *o) {
    o[0] = 0x89; o[1] = 'P'; o[2] = 'N'; o[3] = 'G'; o[4] = 0x0d; o[5] = 0x0a; o[6] = 0x1a; o[7] = 0x0a;
    rtc_png_be32(o + 8, 13);
    o[12] = 'I'; o[13] = 'H'; o[14] = 'D'; o[15] = 'R';
    rtc_png_be32(o + 16, width);
    rtc_png_be32(o + 20, height);
    o[24] = 8;
    o[25] = channels == 4 ? 6 : 2;
    o[26] = o[27] = o[28] = 0;
}

#endif
