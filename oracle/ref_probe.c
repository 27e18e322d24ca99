/*
 * ref_probe.c — TEST INFRASTRUCTURE ONLY. Our own glue, compiled together with the reference's sources
 * (never copied; see oracle/Makefile `ref`) into oracle/_ref/libzultra_ref.so.
 *
 * The reference keeps its intermediates (match[], split offsets, per-sub-block costs and bits) inside
 * `zultra_compressor_t` (src/private.h:64-99). This file includes the reference's own headers to read
 * them, so that the restatement in zultra_oracle.c — and through it the HIP kernels — can be pinned
 * stage by stage, not only on final bytes. Each probe drives exactly the call sequence of
 * zultra_stream_compress (src/libzultra.c:287-343).
 */
#include <stdlib.h>
#include <string.h>
#include "libzultra.h"
#include "private.h"
#include "matchfinder.h"
#include "blockdeflate.h"
#include "huffman/huffutils.h"

typedef struct {
   zultra_stream_t strm;
   int max_block;
   int prev, n;           /* window currently analysed */
   const unsigned char *win;
} ref_probe_t;

ref_probe_t *ref_probe_create(int nMaxBlockSize) {
   ref_probe_t *p = (ref_probe_t *)calloc(1, sizeof(ref_probe_t));
   if (!p) return NULL;
   if (zultra_stream_init(&p->strm, 0, (unsigned int)nMaxBlockSize) != ZULTRA_OK) {
      free(p);
      return NULL;
   }
   p->max_block = (int)p->strm.state->max_block_size;
   return p;
}

void ref_probe_destroy(ref_probe_t *p) {
   if (p) {
      zultra_stream_end(&p->strm);
      free(p);
   }
}

/* libzultra.c:287-293: suffix array + interval tree, skip history, find all matches of the block.
 * win = prev history bytes followed by n block bytes (prev <= 32768, n <= max block). The window pointer
 * must stay valid for later probes. */
int ref_probe_analyse(ref_probe_t *p, const unsigned char *win, int prev, int n) {
   zultra_compressor_t *c = p->strm.state;
   if (prev < 0 || prev > HISTORY_SIZE || n <= 0 || n > p->max_block) return -1;
   if (zultra_build_suffix_array(c, win, prev + n)) return -2;
   if (prev) zultra_skip_matches(c, 0, prev);
   zultra_find_all_matches(c, prev, prev + n);
   p->win = win;
   p->prev = prev;
   p->n = n;
   return 0;
}

/* Copy the match rows of the block positions: out[(i*8+m)*2+0]=length, +1=offset, i relative to block. */
void ref_probe_get_matches(ref_probe_t *p, unsigned short *out) {
   zultra_compressor_t *c = p->strm.state;
   const zultra_match_t *m = c->match + ((size_t)p->prev << MATCHES_PER_OFFSET_SHIFT);
   size_t i, cnt = (size_t)p->n * NMATCHES_PER_OFFSET;
   for (i = 0; i < cnt; i++) {
      out[2 * i] = m[i].length;
      out[2 * i + 1] = m[i].offset;
   }
}

/* libzultra.c:303: block splitter. Returns the number of entries written (last one = prev+n). */
int ref_probe_split(ref_probe_t *p, int *pSplitOffset /* [MAX_SPLITS] */) {
   return zultra_block_split(p->strm.state, p->win, p->prev, p->n, MAX_SPLITS, pSplitOffset);
}

/* libzultra.c:317-324: static / dynamic cost of one sub-block and the resulting type decision. */
int ref_probe_costs(ref_probe_t *p, int nStart, int nSize, int *pStatic, int *pDynamic) {
   zultra_compressor_t *c = p->strm.state;
   int s = 0, d = 0;
   if (zultra_block_prepare_cost_evaluation(c, p->win, nStart, nSize) < 0 ||
       zultra_block_evaluate_static_cost(&c->literalsEncoder, &c->offsetEncoder, &s) < 0 ||
       zultra_huffman_encoder_estimate_dynamic_codelens(&c->literalsEncoder) < 0 ||
       zultra_huffman_encoder_estimate_dynamic_codelens(&c->offsetEncoder) < 0 ||
       zultra_block_evaluate_dynamic_cost(&c->literalsEncoder, &c->offsetEncoder, &d) < 0)
      return -1;
   *pStatic = s;
   *pDynamic = d;
   return (s <= d) ? 0 : 1;   /* nIsDynamic */
}

/* libzultra.c:343: encode one sub-block body (no BFINAL/BTYPE bits) from bit phase 0 into out.
 * Returns 0 and the exact bit count, or -1 when zultra_block_deflate fails. Also copies out the final
 * parse (best_match) when pBest != NULL: pBest[(i-nStart)*2+0]=length, +1=offset. */
int ref_probe_deflate(ref_probe_t *p, int nStart, int nSize, int nIsDynamic,
                      unsigned char *out, int nOutCap, long long *pBits, unsigned short *pBest) {
   zultra_compressor_t *c = p->strm.state;
   zultra_bitwriter_t bw;
   int r, i;

   zultra_bitwriter_init(&bw, out, 0, nOutCap);
   r = zultra_block_deflate(c, &bw, p->win, nStart, nSize, nIsDynamic);
   if (r < 0) return -1;
   *pBits = (long long)bw.nOutOffset * 8 + bw.nEncBitCount;
   if (zultra_bitwriter_flush_bits(&bw) < 0) return -1;
   if (pBest) {
      for (i = 0; i < nSize; i++) {
         pBest[2 * i] = c->best_match[nStart + i].length;
         pBest[2 * i + 1] = c->best_match[nStart + i].offset;
      }
   }
   return 0;
}

/* Final code lengths of the last ref_probe_deflate call (288 lit/len + 32 dist). */
void ref_probe_get_codelens(ref_probe_t *p, int *pLit /*[288]*/, int *pDist /*[32]*/) {
   zultra_compressor_t *c = p->strm.state;
   memcpy(pLit, c->literalsEncoder.nCodeLength, 288 * sizeof(int));
   memcpy(pDist, c->offsetEncoder.nCodeLength, 32 * sizeof(int));
}

/* ---- the entropy stage on given histograms -------------------------------------------------------------
 * The reference's own encoders (huffman/huffencoder.h), their nEntropy set from a histogram instead of a parse, driven
 * through the calls zultra_stream_compress and zultra_block_deflate make on them. The record is the one the oracle's
 * zo_entropy_init / zo_entropy_build and the device's zultra_hip_entropy_probe fill (oracle/zultra_oracle.h). */
typedef struct {
   unsigned char lit_len[288], dist_len[32];
   unsigned short lit_code[288], dist_code[32];
   unsigned char pre_lit_len[288], pre_dist_len[32];
   unsigned int is_dynamic, failed, hdr_bits;
   int static_cost, dynamic_cost;
   unsigned int settled;
   unsigned int reserved[2];
} ref_entropy_rec_t;

static void ref_rec_codes(ref_entropy_rec_t *rec, const zultra_huffman_encoder_t *lit, const zultra_huffman_encoder_t *dist) {
   int i;
   for (i = 0; i < 288; i++) {
      rec->lit_len[i] = (unsigned char)lit->nCodeLength[i];
      rec->lit_code[i] = (unsigned short)(lit->nCodeLength[i] ? lit->nCodeWord[i] : 0);
   }
   for (i = 0; i < 32; i++) {
      rec->dist_len[i] = (unsigned char)dist->nCodeLength[i];
      rec->dist_code[i] = (unsigned short)(dist->nCodeLength[i] ? dist->nCodeWord[i] : 0);
   }
}

static void ref_rec_pre(ref_entropy_rec_t *rec, const zultra_huffman_encoder_t *lit, const zultra_huffman_encoder_t *dist) {
   int i;
   for (i = 0; i < 288; i++) rec->pre_lit_len[i] = (unsigned char)lit->nCodeLength[i];
   for (i = 0; i < 32; i++) rec->pre_dist_len[i] = (unsigned char)dist->nCodeLength[i];
}

/* libzultra.c:317-324, then the start of zultra_block_deflate (blockdeflate.c:832-868), for the tokens tok[0..ntok):
 * literal/length symbol | distance symbol << 9; the end-of-block symbol is added here. */
int ref_probe_entropy_init(const unsigned short *tok, unsigned int ntok, ref_entropy_rec_t *rec) {
   zultra_huffman_encoder_t lit, dist;
   unsigned int t;
   int i, s = 0, d = 0;

   memset(rec, 0, sizeof(*rec));
   if (zultra_huffman_encoder_init(&lit, 288, 15, 0) < 0 || zultra_huffman_encoder_init(&dist, 32, 15, 0) < 0) return -1;
   for (t = 0; t < ntok; t++) {
      int sym = tok[t] & 511;
      if (sym >= 288) return -1;
      lit.nEntropy[sym]++;
      if (sym > 256) dist.nEntropy[(tok[t] >> 9) & 31]++;
   }
   lit.nEntropy[256]++;

   if (zultra_block_evaluate_static_cost(&lit, &dist, &s) < 0 ||
       zultra_huffman_encoder_estimate_dynamic_codelens(&lit) < 0 ||
       zultra_huffman_encoder_estimate_dynamic_codelens(&dist) < 0 ||
       zultra_block_evaluate_dynamic_cost(&lit, &dist, &d) < 0)
      return -1;
   rec->static_cost = s;
   rec->dynamic_cost = d;
   rec->is_dynamic = (s <= d) ? 0 : 1;

   if (!rec->is_dynamic) {
      for (i = 0; i < 288; i++) lit.nCodeLength[i] = i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : 8));   /* RFC 1951 3.2.6 */
      for (i = 0; i < 32; i++) dist.nCodeLength[i] = 5;
      if (zultra_huffman_encoder_build_static_codewords(&lit) < 0 || zultra_huffman_encoder_build_static_codewords(&dist) < 0) rec->failed = 1;
   }
   else {
      if (zultra_huffman_encoder_build_dynamic_codewords(&lit) < 0) rec->failed = 1;
      if (zultra_huffman_encoder_build_dynamic_codewords(&dist) < 0) rec->failed = 1;
   }
   ref_rec_codes(rec, &lit, &dist);
   ref_rec_pre(rec, &lit, &dist);
   return 0;
}

/* What zultra_block_deflate does with the encoders once a parse pass has counted its symbols (blockdeflate.c:893-919), and
 * after the last pass up to the token bits (:925-992), for the histogram hist[320] (288 + 32, without the end-of-block
 * symbol). Passes 0..2 also say whether the lengths the next pass would price with (:873-881) are in_force[320]. */
int ref_probe_entropy_build(const unsigned int *hist, int pass, const unsigned char *in_force, ref_entropy_rec_t *rec,
                            unsigned char *hdr, int cap) {
   zultra_huffman_encoder_t lit, dist, alt_lit, alt_dist, tables;
   zultra_bitwriter_t bw;
   int lens[288 + 32];
   int i, nlit, ndist, ncl, cur = 0, alt = 0, mask, best_mask = -1, best_cost = 0;

   memset(rec, 0, sizeof(*rec));
   rec->is_dynamic = 1;
   if (zultra_huffman_encoder_init(&lit, 288, 15, 0) < 0 || zultra_huffman_encoder_init(&dist, 32, 15, 0) < 0) return -1;
   for (i = 0; i < 288; i++) lit.nEntropy[i] = (int)hist[i];
   for (i = 0; i < 32; i++) dist.nEntropy[i] = (int)hist[288 + i];
   lit.nEntropy[256]++;

   if (pass == 3) {
      int used = 0;
      for (i = 0; used < 2 && i < 30; i++)
         if (dist.nEntropy[i]) used++;
      if (used == 0)
         dist.nEntropy[0] = dist.nEntropy[1] = 1;
      else if (used == 1)
         dist.nEntropy[dist.nEntropy[0] ? 1 : 0] = 1;
   }
   if (zultra_huffman_encoder_build_dynamic_codewords(&lit) < 0) rec->failed = 1;
   if (zultra_huffman_encoder_build_dynamic_codewords(&dist) < 0) rec->failed = 1;

   if (pass < 3) {
      int moved = 0;
      for (i = 0; i < 288; i++) moved |= (lit.nCodeLength[i] ? lit.nCodeLength[i] : 9) != (in_force[i] ? in_force[i] : 9);
      for (i = 0; i < 32; i++) moved |= (dist.nCodeLength[i] ? dist.nCodeLength[i] : 6) != (in_force[288 + i] ? in_force[288 + i] : 6);
      rec->settled = (!moved && !rec->failed) ? 1 : 0;
      ref_rec_codes(rec, &lit, &dist);
      return 0;
   }
   ref_rec_pre(rec, &lit, &dist);

   /* the RLE-friendlier alternative, kept only when it is cheaper overall */
   alt_lit = lit;
   alt_dist = dist;
   zultra_block_evaluate_dynamic_cost(&alt_lit, &alt_dist, &cur);
   zultra_huffman_encoder_optimize_for_rle(288, alt_lit.nEntropy, lens);
   zultra_huffman_encoder_optimize_for_rle(32, alt_dist.nEntropy, lens);
   if (zultra_huffman_encoder_build_dynamic_codewords(&alt_lit) < 0 || zultra_huffman_encoder_build_dynamic_codewords(&alt_dist) < 0) {
      rec->failed = 1;
      ref_rec_codes(rec, &lit, &dist);
      return 0;
   }
   zultra_block_evaluate_dynamic_cost(&alt_lit, &alt_dist, &alt);
   if (alt < cur) {
      lit = alt_lit;
      dist = alt_dist;
   }
   ref_rec_codes(rec, &lit, &dist);

   /* the code-length mask that gives the smallest tables; among equals the last one tried */
   nlit = zultra_huffman_encoder_get_defined_var_lengths_count(&lit, 257);
   ndist = zultra_huffman_encoder_get_defined_var_lengths_count(&dist, 1);
   memcpy(lens, lit.nCodeLength, nlit * sizeof(int));
   memcpy(lens + nlit, dist.nCodeLength, ndist * sizeof(int));
   zultra_huffman_encoder_init(&tables, 19, 7, 0);
   for (mask = 0; mask <= MAX_CODES_MASK; mask += (mask >= 7) ? 2 : 1) {
      int cost;
      zultra_huffman_encoder_update_var_lengths_entropy(&tables, nlit + ndist, lens, mask);
      zultra_huffman_encoder_build_dynamic_codewords(&tables);
      cost = zultra_huffman_encoder_get_var_lengths_size(&tables, nlit + ndist, lens, mask);
      if (best_mask == -1 || best_cost >= cost) {
         best_mask = mask;
         best_cost = cost;
      }
      for (i = 0; i < 19; i++) tables.nEntropy[i] = 0;
   }
   zultra_huffman_encoder_update_var_lengths_entropy(&tables, nlit + ndist, lens, best_mask);
   zultra_huffman_encoder_build_dynamic_codewords(&tables);

   ncl = zultra_huffman_encoder_get_raw_table_size(&tables);
   zultra_bitwriter_init(&bw, hdr, 0, cap);
   if (nlit > 286 || ndist > 30 || ncl > 19 ||
       zultra_bitwriter_put_bits(&bw, nlit - 257, 5) < 0 || zultra_bitwriter_put_bits(&bw, ndist - 1, 5) < 0 ||
       zultra_bitwriter_put_bits(&bw, ncl - 4, 4) < 0 ||
       zultra_huffman_encoder_write_raw_table(&tables, 3, ncl, &bw) < 0 ||
       zultra_huffman_encoder_write_var_lengths(&tables, nlit + ndist, lens, best_mask, &bw) < 0) {
      rec->failed = 1;
      return 0;
   }
   rec->hdr_bits = (unsigned int)(bw.nOutOffset * 8 + bw.nEncBitCount);
   if (zultra_bitwriter_flush_bits(&bw) < 0) rec->failed = 1;
   return 0;
}

/* Whole-stream entry with a preset dictionary (libzultra.c:177 + 601), for dictionary fixtures. */
size_t ref_probe_memory_compress_dict(const unsigned char *in, size_t nIn, unsigned char *out, size_t nOutCap,
                                      unsigned int nFlags, unsigned int nMaxBlockSize,
                                      const void *pDict, int nDictSize) {
   zultra_stream_t strm;
   zultra_status_t st;
   memset(&strm, 0, sizeof(strm));
   if (zultra_stream_init(&strm, nFlags, nMaxBlockSize)) return (size_t)-1;
   if (pDict && nDictSize > 0 && zultra_stream_set_dictionary(&strm, pDict, nDictSize) != ZULTRA_OK) {
      zultra_stream_end(&strm);
      return (size_t)-1;
   }
   strm.next_in = in;
   strm.avail_in = nIn;
   strm.next_out = out;
   strm.avail_out = nOutCap;
   st = zultra_stream_compress(&strm, ZULTRA_FINALIZE);
   zultra_stream_end(&strm);
   if (st != ZULTRA_STREAM_END) return (size_t)-1;
   return nOutCap - strm.avail_out;
}
