/*
 * zultra_hip.h — C ABI of the MI355X (gfx950) device layer: batches of independent max-blocks in, per-sub-block
 * deflate bit strings out. Plain pointers and sizes only.
 *
 * This is the inner boundary of the reference: the five calls that zultra_stream_compress makes per max-block
 * (reference src/libzultra.c:287-343)
 *      zultra_build_suffix_array(win, prev+n)            :287   \
 *      zultra_skip_matches(0, prev)                      :291    >  stage 1  (zultra_hip: match rows)
 *      zultra_find_all_matches(prev, prev+n)             :293   /
 *      zultra_block_split(win, prev, n, 64, splits)      :303      stage 2  (zultra_hip: sub-block boundaries)
 *      zultra_block_prepare_cost_evaluation / _evaluate_static_cost / 2x _estimate_dynamic_codelens /
 *      _evaluate_dynamic_cost                            :317-321  stage 3a (static vs dynamic)
 *      zultra_block_deflate(win, start, size, isDynamic) :343      stage 3b (bits of the sub-block body)
 * are replaced by ONE batched call, zultra_hip_compress_blocks(), which runs them for many max-blocks at once
 * (max-blocks are independent given their 32 KiB of raw history). What stays on the caller's side
 * is exactly what depends on the running bit phase of the output stream: BFINAL/BTYPE bits, the stored-block
 * fallback and the bit carry between max-blocks (libzultra.c:327-398, 414-436) — done by zultra_hip_stitch().
 *
 * There is no CPU fallback: every entry point fails (NULL / negative) when no HIP device is usable.
 */
#ifndef ZULTRA_HIP_H
#define ZULTRA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zultra_hip_ctx_s zultra_hip_ctx_t;

/* One max-block: window = data + win_off, `prev` bytes of history (0..32768) followed by `n` block bytes
 * (1..max_block_size). Mirrors the (pInWindow, nPreviousBlockSize, nInDataSize) triple of libzultra.c:287-303. */
typedef struct zultra_hip_block_s {
   uint64_t win_off;
   uint32_t prev;
   uint32_t n;
} zultra_hip_block_t;

/* One sub-block result, in stream order. Mirrors what libzultra.c:314-347 needs to frame it. */
typedef struct zultra_hip_subblock_s {
   uint32_t block;          /* index of the max-block in the batch */
   uint32_t start;          /* offset of the sub-block inside the max-block (nInStart, libzultra.c:297) */
   uint32_t size;           /* nBlockSize, libzultra.c:314 */
   uint32_t is_dynamic;     /* nIsDynamic, libzultra.c:323-324 */
   int32_t static_cost;     /* nStaticCost  (blockdeflate.c:538) */
   int32_t dynamic_cost;    /* nDynamicCost (blockdeflate.c:577) */
   uint32_t failed;         /* non-zero: zultra_block_deflate would have failed / outgrown its buffer -> store it */
   uint32_t reserved;
   uint64_t nbits;          /* exact bit length of the body (after the 3 header bits) */
   uint64_t bits_off;       /* byte offset of the body's bit string (bit phase 0) in the payload */
} zultra_hip_subblock_t;

/* Timings of the last batch, milliseconds, measured with HIP events on the context's stream. */
typedef struct zultra_hip_timing_s {
   float h2d_ms, matchfinder_ms, tokenize_split_ms, encode_ms, d2h_ms, total_ms;
   float group_ms, frontier_ms, stitch_ms;
   float init_ms, parse_ms, build_ms, post_ms, emit_ms;   /* parts of encode_ms: planning + zh_sb_init + zh_list_huge, 4 x the parse kernels, 4 x zh_sb_build, zh_post_tasks, zh_emit_tasks
                                                              (a batch runs as staggered runs on streams of their own: each figure is the SUM over the runs, which overlap in wall time) */
   float head_ms;                                          /* wall time from the batch's first launch to the end of the FIRST run's matchfinder: nothing of the batch can overlap it */
   float tail_ms;                                          /* wall time from the end of the LAST run's matchfinder to the batch's last completion: token chain, splitter, four parse / rebuild
                                                              rounds, literalisation, emission — it does not shrink with the batch (the strong-scaling floor) */
} zultra_hip_timing_t;

/* Number of usable HIP devices (0 if none). */
int zultra_hip_device_count(void);

/* Device self-check of the wave64 primitives the kernels rely on (DPP row reductions, readlane, prefix sums)
 * against plain LDS arithmetic. Returns 0 when they agree, a positive count of mismatches, negative on HIP errors. */
int zultra_hip_selftest(void);

/* Diagnostics: the kernels that build a sub-block's Huffman codes (zh_sb_init, zh_sb_build), run as they ship on `n` made-up
 * sub-blocks — the test-suite compares them with the reference on histograms that no input would be found for. Needs no context.
 *   mode INIT : sub-block i owns the tokens [tok_off[i], tok_off[i + 1]) of tok_info (one uint16 per token: literal/length symbol
 *               below 288 | distance symbol << 9); the kernel takes their histogram, adds the end-of-block symbol, prices the
 *               static and the dynamic form, and builds the first codes.
 *   mode BUILD: sub-block i owns rows [i * ntasks, (i + 1) * ntasks) of hist_part, ZULTRA_HIP_ENTROPY_NSYM counts each (288
 *               literal/length, 32 distance), which the kernel sums and adds the end-of-block symbol to; `pass` is 0..3 (3 = the
 *               last: distance-code fix, RLE-friendly alternative, block header); in_force holds 320 code lengths per sub-block,
 *               the ones a pass before would have left (passes 0..2 compare theirs with them: `settled`).
 * Sub-blocks [0, grid) are worked on by the one-per-workgroup form of the kernel and [grid, n) by the striding form (1 <= grid <= n).
 * recs[n] receives the coder states (codes of symbols without a length are undefined), slots[n * ZULTRA_HIP_ENTROPY_SLOT] the
 * header bits of each sub-block (zero beyond hdr_bits), settled[2] — may be NULL — the run's two counters of settled sub-blocks
 * (passes saved; the same weighted by the sub-block's KiB, which the probe sets to one). Returns 0, or a negative error. */
#define ZULTRA_HIP_ENTROPY_INIT 0
#define ZULTRA_HIP_ENTROPY_BUILD 1
#define ZULTRA_HIP_ENTROPY_NSYM 320
#define ZULTRA_HIP_ENTROPY_SLOT 1024
typedef struct zultra_hip_entropy_rec_s {
   uint8_t lit_len[288], dist_len[32];
   uint16_t lit_code[288], dist_code[32];
   uint8_t pre_lit_len[288], pre_dist_len[32];   /* lengths of the last pass before the RLE-friendly alternative */
   uint32_t is_dynamic, failed, hdr_bits;
   int32_t static_cost, dynamic_cost;
   uint32_t settled;
   uint32_t reserved[2];
} zultra_hip_entropy_rec_t;
int zultra_hip_entropy_probe(int mode, uint32_t n, uint32_t grid, int pass, uint32_t ntasks, const uint32_t *hist_part, const uint8_t *in_force,
                             const uint16_t *tok_info, const uint32_t *tok_off, zultra_hip_entropy_rec_t *recs, uint8_t *slots, uint32_t *settled);

/* Diagnostics: a streaming 4-byte-per-lane copy of `nbytes`, used to calibrate the rocprofv3 FETCH_SIZE / WRITE_SIZE
 * counters for this access width (profiles/, tools/pmc_traffic.py). Returns 0 on success. */
int zultra_hip_traffic_probe(size_t nbytes);

/* The second roofline denominator: measured bandwidth of a 16-byte-per-lane streaming copy of `nbytes`,
 * `iters` launches timed with HIP events on the null stream. Returns GB/s (bytes read + bytes written), negative on errors. */
double zultra_hip_copy_bandwidth(size_t nbytes, int iters);

/* Create a context on `device` able to take batches of up to max_blocks max-blocks of up to max_block_size bytes
 * (clamped like libzultra.c:87-92). All device memory is allocated here and released by zultra_hip_destroy
 * (the reference allocates in zultra_stream_init and frees in zultra_stream_end, libzultra.c:82-166,521-565).
 * Returns NULL on failure (no device, out of memory). */
zultra_hip_ctx_t *zultra_hip_create(int device, uint32_t max_block_size, uint32_t max_blocks);
void zultra_hip_destroy(zultra_hip_ctx_t *ctx);
const char *zultra_hip_last_error(const zultra_hip_ctx_t *ctx);

/* What a context was created with, and the device memory it holds (any pointer may be NULL). */
void zultra_hip_ctx_info(const zultra_hip_ctx_t *ctx, int *device, uint32_t *max_block_size, uint32_t *max_blocks, size_t *device_bytes);
/* Device bytes zultra_hip_create(device, max_block_size, max_blocks) will allocate, computed from the same layout without
 * allocating: callers size their batches against the memory they want to spend. */
size_t zultra_hip_context_bytes_on(int device, uint32_t max_block_size, uint32_t max_blocks);
size_t zultra_hip_context_bytes(uint32_t max_block_size, uint32_t max_blocks);   /* ... on the calling thread's current device */

/* Pinned host staging owned by the context (which: 0 = input side, 1 = output side), at least `size` bytes, valid until
 * the context is destroyed or a larger size is requested. The streaming API stages caller data through these: copies
 * from pageable memory run at a fraction of the PCIe rate. Returns NULL on failure. */
void *zultra_hip_staging(zultra_hip_ctx_t *ctx, int which, size_t size);

/* Bytes of input the context can hold per batch (max_blocks * max_block_size + 32768 of leading history). */
size_t zultra_hip_data_capacity(const zultra_hip_ctx_t *ctx);

/* Run stages 1-3 for a batch. `data` holds every window of the batch: host memory if data_on_device == 0 (uploaded in one piece:
 * best from pinned memory, e.g. zultra_hip_staging), a device pointer valid on the context's device if 1 (read in place, nothing
 * is copied), pageable host memory if 2 (staged through the context's pinned buffer and uploaded run by run, each run's bytes
 * under the kernels of the run before it). Returns the number of sub-blocks (>0) or a negative error. Results stay in the context
 * until the next batch. */
int zultra_hip_compress_blocks(zultra_hip_ctx_t *ctx, const void *data, size_t data_size, int data_on_device,
                               const zultra_hip_block_t *blocks, uint32_t nblocks);

/* Results of the last batch as host pointers owned by the context (valid until the next batch / destroy). */
const zultra_hip_subblock_t *zultra_hip_subblocks(const zultra_hip_ctx_t *ctx, uint32_t *count);
const uint8_t *zultra_hip_payload(const zultra_hip_ctx_t *ctx, size_t *size);
void zultra_hip_last_timing(const zultra_hip_ctx_t *ctx, zultra_hip_timing_t *t);

/* Shape of the last batch: how the parse was decomposed. huge_* = tasks (and their positions) that hold a
 * barrier-free run too long for the four-recurrences-per-wave kernel and went to the single-chain kernel instead. */
typedef struct zultra_hip_stats_s {
   uint64_t positions, huge_positions;
   uint32_t blocks, subblocks, tasks, huge_tasks;
   uint32_t cut_tasks, cut_segments;   /* chain tasks parsed as speculative segments, and their segments */
   uint32_t cut_redone;                /* segments whose speculated costs did not match and were parsed again (sum over the passes) */
   uint32_t runs;                      /* staggered runs the batch was cut into (ZULTRA_HIP_STREAMS, fewer for small batches) */
   uint32_t settled_passes;            /* (sub-block, parse pass) pairs not run: the sub-block's code lengths had reached a fixed point of the loop at
                                          blockdeflate.c:874-901, every further pass would have reproduced the parse it has */
   uint32_t settled_kib;               /* ... the input they cover, in KiB (of 4 x positions / 1024 for the four passes of everything) */
   uint32_t cut_demoted;               /* cut tasks that had several failed cuts in one pass and were parsed as one chain in the passes left */
   uint32_t runs_without_chain_kernels;   /* runs of the last batch enqueued without zh_parse_chain: their counterparts in the context's batch before it listed no chains (round 6) */
   uint32_t batches_rerun;                /* batches of this context run a second time because such a run listed chains after all (since the context was created) */
   uint32_t runs_fitted;                  /* diagnostics, decides nothing: at its creation a context that picks the run count itself lets the streams of its runs (three at most) spin
                                             side by side once; the largest number of runs, from the first, whose streams all had hardware queues of their own (1: not even two). A context
                                             that does not look (files, ZULTRA_HIP_STREAMS set, a largest batch of one run) reports the runs it created streams for, three at most */
   uint32_t stream_collisions;            /* ... and the pairs of those streams that shared a queue at that look (0: every run of a batch below 256 MiB can overlap the others) */
} zultra_hip_stats_t;
void zultra_hip_last_stats(const zultra_hip_ctx_t *ctx, zultra_hip_stats_t *out);

/* The number of staggered runs a batch of nblocks max-blocks and batch_bytes input bytes is cut into (pure: no context, no device). streams_setting: ZULTRA_HIP_STREAMS
 * (0: not set). A positive setting asks for that many runs, otherwise three, four from 256 MiB on; either way a run has at least four max-blocks and 4 MiB, and a batch
 * at least one run. */
uint32_t zultra_hip_runs_for(uint64_t batch_bytes, uint32_t nblocks, int streams_setting);

/* Diagnostics: the matchfinder's chunk size in this context for a segment window of window_size bytes (history + block + look-ahead) — a bigram class of
 * that many positions or more is refined through device memory by a kernel of its own, from a note —, and in *max_notes (may be NULL) how many such
 * classes one segment's note table holds. 0 without a context. */
uint32_t zultra_hip_mf_chunk(const zultra_hip_ctx_t *ctx, uint32_t window_size, uint32_t *max_notes);

/* Diagnostics: with ZULTRA_HIP_CHAIN_TRACE=1 in the environment when the context is created, the chain kernels record per work
 * ticket {positions, start, end} on the device's 100 MHz clock; out = uint64[4 runs][4 passes][*slots][3]. Returns 0, or -1 when
 * tracing is off. */
int zultra_hip_chain_trace(zultra_hip_ctx_t *ctx, uint64_t *out, uint32_t *slots);

/* Diagnostics: the tasks of run `run` of the last batch that were cut into speculative segments, four words each: task index in
 * the run, number of segments K | (segment length / 32) << 12, first cost-vector slot, segment completions | (cuts that failed their check and
 * were parsed again) << 16, both counted over the four passes. Returns the number of entries written (at most cap), -1 on error. */
int zultra_hip_cut_tasks(zultra_hip_ctx_t *ctx, uint32_t run, uint32_t *out, uint32_t cap);

/* Stage outputs of the last batch, for parity tests (copied device -> host on request).
 *   matches: n*8 entries {u16 length, u16 offset} of max-block `block`          (match[], private.h:59-62,97)
 *   splits : absolute window offsets of the sub-block ends, last = prev+n; returns the count (nSplitOffset, libzultra.c:299)
 *   parse  : n entries {u16 length, u16 offset}, the final parse                (best_match[], private.h:98) */
int zultra_hip_get_matches(zultra_hip_ctx_t *ctx, uint32_t block, uint16_t *out);
int zultra_hip_get_splits(zultra_hip_ctx_t *ctx, uint32_t block, int *out /* [64] */);
int zultra_hip_get_parse(zultra_hip_ctx_t *ctx, uint32_t block, uint16_t *out);

/*
 * Stitcher (host): appends the framed sub-blocks of a batch to a deflate stream, reproducing libzultra.c:327-398
 * (3 header bits, compressed-or-stored decision from the running bit phase, stored pieces of <= 65535 bytes) and
 * the bit carry across max-blocks (:427-434).
 *   state        : running bit writer (zero-initialise before the first batch of a stream)
 *   raw          : the raw bytes of the batch's max-blocks, max-block b at raw + raw_off[b] (for stored sub-blocks)
 *   final_block  : index of the max-block that ends the stream (ZULTRA_FINALIZE and no more input), or -1
 * Writes whole bytes to out (capacity out_cap) and returns the number written, or (size_t)-1 on overflow / error
 * (the reference's ZULTRA_ERROR_DST). With out == NULL nothing is written: the call only advances `state` and returns
 * the byte count, which is how a rank learns at which bit offset its shard starts (multi-GPU).
 * `state` may start at any phase 0..7 with acc = 0: the first byte then carries only this shard's bits. Call zultra_hip_stitch_finish() after the last batch to pad to a byte
 * (libzultra.c:414-417).
 */
typedef struct zultra_hip_bitstate_s {
   uint32_t acc;     /* pending bits, LSB first (zultra_bitwriter_t.nEncBitsData, bitwriter.h:27-33) */
   uint32_t nacc;    /* 0..7             (nEncBitCount) */
} zultra_hip_bitstate_t;

size_t zultra_hip_stitch(zultra_hip_bitstate_t *state, const zultra_hip_subblock_t *subs, uint32_t nsubs,
                         const uint8_t *payload, const uint8_t *raw, const uint64_t *raw_off, uint32_t max_block_size,
                         int final_block, uint8_t *out, size_t out_cap);
size_t zultra_hip_stitch_finish(zultra_hip_bitstate_t *state, uint8_t *out, size_t out_cap);

/*
 * Stitcher (device): same result as zultra_hip_stitch for the last batch, with nothing on the host: a scan kernel takes the
 * phase-dependent decisions of libzultra.c:327-398 from the 48-byte descriptors (a transfer table bit phase -> bits added
 * per run of max-blocks, composed across the batch), a second kernel moves the bits; the stream stays in HBM.
 *   state->nacc : pending bits (0..7) before the batch; updated to the pending bits after it (state->acc is not used:
 *                 the caller ORs its pending bits into byte 0 of the result, and reads the new partial byte back).
 *   *end_bit    : bits from the start of byte 0 to the end of the batch; the buffer holds ceil(end_bit/8) bytes.
 * Returns 0, -2 where the reference fails with ZULTRA_ERROR_DST, -1 on HIP errors.
 */
int zultra_hip_stitch_device(zultra_hip_ctx_t *ctx, zultra_hip_bitstate_t *state, int final_block, uint64_t *end_bit);
/*
 * The next batch of max-blocks (zultra_hip_compress_blocks) is stitched at bit phase `phase` (0..7; final_block as for zultra_hip_stitch_device) right behind
 * its last kernel, before the host is woken: a caller that knows the phase its batch starts at — every batch of a stream compressed batch by batch
 * (libzultra.c:327-398 carries the phase from max-block to max-block), the first job of zultra_memory_compress — saves the second synchronisation. The
 * zultra_hip_stitch_device call that follows with the same phase and final_block returns that stitch's result without launching anything; with other
 * arguments it stitches again. The setting is consumed by one batch. enable = 0 disarms. Returns 0, -1 for a files context.
 */
int zultra_hip_stitch_with_batch(zultra_hip_ctx_t *ctx, int enable, uint32_t phase, int final_block);
/*
 * Where the last batch would end for each of the eight bit phases it could start at (the same scan, nothing written):
 * end_bits[p] counts from the start of the byte that holds the p pending bits; bit p of *failed_mask is set where the
 * reference would fail with ZULTRA_ERROR_DST from that phase. What a device hands its neighbours when one stream
 * (libzultra.c:601-619) is cut over several of them: a shard's bit length depends on the phase it starts at.
 */
int zultra_hip_stitch_phase_table(zultra_hip_ctx_t *ctx, uint64_t *end_bits /* 8 */, uint32_t *failed_mask);   /* (rewrites the last stitch's items and report: stitch again before reading the stream) */
const void *zultra_hip_stream_device(const zultra_hip_ctx_t *ctx);
int zultra_hip_stream_read(zultra_hip_ctx_t *ctx, void *out, size_t offset, size_t nbytes);
/* Counterpart of zultra_hip_stream_read: overwrite bytes of the stream buffer (diagnostics; what the verify tests corrupt a stream with). */
int zultra_hip_stream_write(zultra_hip_ctx_t *ctx, const void *in, size_t offset, size_t nbytes);

/*
 * Verification: the device inflates the stream it has just assembled and compares it with the batch's input — one wave per
 * sub-block, each from its own first header bit; a literal must equal the input byte, a match must copy what the input has, every sub-block's
 * decode must end where the next one starts, BFINAL must sit on the stream's last block and nowhere else. Any content of the stream buffer
 * gives a verdict.
 */
#define ZULTRA_HIP_VERIFY_OK 0          /* reasons: 1 header, 2 code lengths, 3 symbol, 4 distance, 5 literal differs, 6 match differs,
                                           7 stored LEN/NLEN, 8 stored bytes differ, 9 size overrun, 10 end bit, 11 BFINAL, 12 stream end */
typedef struct zultra_hip_verify_s {
   uint32_t bad_subblocks;   /* sub-blocks that did not verify */
   uint32_t first_bad;       /* stream-order index of the first, 0xFFFFFFFF if none */
   uint32_t reason;          /* of first_bad */
   uint32_t block;           /* its max-block */
   uint64_t input_off;       /* offset inside that max-block where it went wrong */
   uint64_t stream_bit;      /* bit of the stream buffer the decoder had reached */
   uint64_t verified_bytes;  /* input bytes of the sub-blocks that verified */
} zultra_hip_verify_t;

/* Inflate-and-compare of the stream the last stitch left in the context's stream buffer (zultra_hip_stitch_device, the stitch armed with
 * zultra_hip_stitch_with_batch, zultra_hip_compress_files / zultra_hip_stitch_files) against the batch's input. 0 = every sub-block
 * verified, 1 = report->bad_subblocks > 0, -1 = HIP error or nothing stitched (a stitch that reported failure, a phase-table call since).
 * The input is read where the batch's kernels read it: the context's own copy for data_on_device 0 and 2; for data_on_device 1 the CALLER'S
 * device pointer, which must therefore stay valid and unchanged until this call returns. */
int zultra_hip_verify_device(zultra_hip_ctx_t *ctx, zultra_hip_verify_t *report);
/* Device time of the last zultra_hip_verify_device's kernel, milliseconds (HIP events on the context's stream). */
float zultra_hip_last_verify_ms(const zultra_hip_ctx_t *ctx);

/*
 * Batched inflate: many independent raw deflate streams (RFC 1951) decoded on the device, one wave64 per stream. Item i is the
 * complete stream at src + src_off (any byte address, any number of stored / fixed / dynamic blocks up to and including the block with BFINAL) and
 * is written to dst + dst_off, at most dst_cap bytes. One stream runs at the speed of ONE wave — a serial chain of tokens —, so the call pays for
 * batches of many streams (the records of a files batch); decoding one large stream in parallel is not what it does. Without a preset dictionary
 * (zultra_hip_inflate_streams_dict below) a match that reaches in front of the item's own output fails with reason 4.
 *   reason   : 0 ok; as for verification where it fits — 1 header (BTYPE 3, HLIT / HDIST out of range), 2 code lengths, 3 symbol, 4 distance (no such
 *              code, symbols 30 and 31, a distance that reaches in front of the item's output), 7 stored LEN/NLEN, 12 the stream ends before its
 *              final block does (bytes behind src_size read as zero); and 13 = the output does not fit in dst_cap
 *   blocks   : deflate blocks decoded
 *   out_size : bytes written (on failure: before the failure); never more than dst_cap, and nothing outside the item's range is touched
 *   src_used : bytes of the item consumed, up to and including the byte that holds the last bit of the final block
 * With *_on_device == 1 the pointer is a device pointer valid on `device` and is used in place, nothing is copied: src = zultra_hip_stream_device(ctx)
 * with the file_off array of zultra_hip_compress_files turned into items inflates a files batch without its bytes leaving the device. With
 * *_on_device == 0 the call stages through device memory it allocates and frees itself (of a host dst only the out_size bytes of every item are
 * written). No context is needed. kernel_ms (may be NULL): device time of the kernel, HIP events.
 * Returns the number of items whose reason is not 0 (0: all of them decoded), or -1 for HIP errors and bad arguments: n == 0, an item range outside
 * src_size or dst_size, destination ranges that overlap. Any bytes in src give a verdict per item and nothing else.
 */
#define ZULTRA_HIP_INFLATE_OK 0
#define ZULTRA_HIP_INFLATE_DST_FULL 13
typedef struct zultra_hip_inflate_item_s { uint64_t src_off, src_size, dst_off, dst_cap; } zultra_hip_inflate_item_t;
typedef struct zultra_hip_inflate_result_s { uint32_t reason, blocks; uint64_t out_size, src_used; } zultra_hip_inflate_result_t;
int zultra_hip_inflate_streams(int device, const void *src, size_t src_size, int src_on_device, void *dst, size_t dst_size, int dst_on_device,
                               const zultra_hip_inflate_item_t *items, uint32_t n, zultra_hip_inflate_result_t *results /* host, n */,
                               float *kernel_ms /* may be NULL */);
/* The same with ONE preset dictionary for every item of the call (records compressed against a shared dictionary: zultra_memory_compress_dict,
 * zlib's deflateSetDictionary): the last min(dict_size, 32768) bytes of dict, at any byte address, lie in front of every item's output as history,
 * which is what zlib's inflateSetDictionary keeps. Reason 4 is then a distance above 32768 or above out_size-so-far + that history length (zlib's
 * "invalid distance too far back"). The history is only read. dict_on_device == 0: staged through device memory the call owns, like src; == 1: used
 * in place, and a dictionary that overlaps an item's destination range (both on the device) is refused with -1, as is dict == NULL with
 * dict_size > 0. dict_size == 0 (dict may be NULL) is zultra_hip_inflate_streams. Items, results, reasons and the return value are the same. */
int zultra_hip_inflate_streams_dict(int device, const void *src, size_t src_size, int src_on_device, void *dst, size_t dst_size, int dst_on_device,
                                    const void *dict, size_t dict_size, int dict_on_device,
                                    const zultra_hip_inflate_item_t *items, uint32_t n, zultra_hip_inflate_result_t *results /* host, n */,
                                    float *kernel_ms /* may be NULL */);

/*
 * Batched inflate of gzip (RFC 1952) and zlib (RFC 1950) MEMBERS with the checks on the device: item i holds one member — header,
 * deflate stream, trailer — at src + src_off; its bytes are decoded to dst + dst_off and their CRC-32 / Adler-32 is taken there and compared with the
 * trailer. Nothing but the results crosses to the host. Three launches on one stream, one synchronisation: zh_frame_heads parses the headers and
 * writes the items of the inflate kernel, zh_inflate_streams[_dict] decodes, zh_check_members sums the output and reads the trailers.
 *   framing  : 0 (raw: exactly zultra_hip_inflate_streams[_dict]'s results, head_size = check = 0), ZULTRA_FLAG_ZLIB_FRAMING or ZULTRA_FLAG_GZIP_FRAMING
 *              (libzultra.h) for ALL items of the call; both bits, or any other bit, is -1
 *   reason   : in this order — 14 the header (gzip: magic, CM, a reserved FLG bit, FHCRC; zlib: CM, CINFO > 7, the CMF/FLG check, FDICT / DICTID; a
 *              header that does not end inside the item); 1..13 the inflate kernel's own reason, out_size as it left it; 12 also where the
 *              trailer does not fit in the item (the member is cut off); 15 the checksum of the output differs from the trailer's; 16 gzip's ISIZE
 *              differs from out_size mod 2^32
 *   src_used : header + deflate stream + trailer. Bytes of the item behind the member's trailer are NOT an error: compare src_used with src_size, or
 *              walk a concatenation of gzip members call by call
 *   head_size: bytes of header; check: the checksum COMPUTED over the output, whenever the stream decoded (0 for raw)
 * gzip: FEXTRA, FNAME and FCOMMENT are skipped, and FHCRC is CHECKED — the low 16 bits of the CRC-32 of the header bytes in front of it, as zlib's
 * inflate does. This is stricter than zultra_memory_decompress, which skips the two bytes.
 * zlib: a header with FDICT must carry the Adler-32 of the WHOLE dictionary as its DICTID (the library's convention, libzultra.h); FDICT without a
 * dictionary, or another DICTID, is 14. And where the call HAS a dictionary a zlib item WITHOUT FDICT is 14 as well — unlike
 * zultra_memory_decompress_dict, which ignores the dictionary for such a stream: the dictionary kernel has one history length per launch, and
 * decoding the item with the history visible would accept "distance too far back" streams that zlib rejects. Such items belong in a call without a
 * dictionary. Raw and gzip items take the dictionary as history, as in zultra_hip_inflate_streams_dict.
 * Items, argument checks, the *_on_device meanings, the dictionary rules and the return value (items with reason != 0; -1 for bad arguments and HIP
 * errors) are those of zultra_hip_inflate_streams_dict. kernel_ms (may be NULL): device time of the three launches — frame, inflate, check.
 */
#define ZULTRA_HIP_INFLATE_BAD_FRAME 14
#define ZULTRA_HIP_INFLATE_BAD_CHECK 15
#define ZULTRA_HIP_INFLATE_BAD_ISIZE 16
typedef struct zultra_hip_member_result_s {
   uint32_t reason, blocks;
   uint64_t out_size, src_used;
   uint32_t head_size, check;
} zultra_hip_member_result_t;
int zultra_hip_inflate_members(int device, const void *src, size_t src_size, int src_on_device, void *dst, size_t dst_size, int dst_on_device,
                               const void *dict, size_t dict_size, int dict_on_device, unsigned int framing,
                               const zultra_hip_inflate_item_t *items, uint32_t n, zultra_hip_member_result_t *results /* host, n */,
                               float *kernel_ms /* [3], may be NULL */);

/*
 * A whole BGZF / multi-member gzip FILE: the device finds the members itself, so the caller names no offsets. A HINTED member starts at p when
 * src_size - p >= 12, src[p..p+3) = 1f 8b 08, FEXTRA is set, XLEN fits in the source, the extra field's subfields reach one with SI1 'B', SI2 'C', SLEN 2 (a
 * subfield that runs past XLEN ends the walk), and L = le16(its data) + 1 has L >= 12 + XLEN + 8 and p + L <= src_size: the member is src[p .. p + L), its
 * ISIZE the last four of those bytes. The index is the chain of hinted members from p = 0: item i = {p_i, L_i, the sum of the ISIZEs before it, ISIZE_i}. It
 * checks nothing else of a member: that is zultra_hip_inflate_members' business, with its reasons 1..16.
 *   stop           : why the chain ended at src_used — 0 the end of the source; 1 magic and CM = 8 but no hint (a gzip member the index cannot size); 2 a hint
 *                    whose L is too short or reaches past the source; 3 anything else (fewer than 12 bytes, no magic); and 4 = more members than `cap` /
 *                    `results_cap`, or more output than dst_size: nothing was written, members / out_size say how much room the file needs
 *   tiles, tiles_rewalked : diagnostics — the source is indexed in tiles of ZULTRA_HIP_INDEX_TILE bytes (environment, any value >= 32; default 256 KiB), each
 *                    from a guessed entry; tiles the chain entered, and those of them whose guess was not the chain's entry and were walked again
 * zultra_hip_index_members: the index alone. items (host, cap entries) may be NULL with cap 0 to learn members and out_size. Returns 0; -1 for bad arguments
 * (src NULL, src_size 0, a bad device, items NULL with cap > 0), HIP errors, and stop 4 (res filled, no item written). kernel_ms (may be NULL): the index kernels.
 * zultra_hip_inflate_file: index, headers, inflate and checks of the indexed members, gzip framing, no dictionary; the items never leave the device except for
 * one read of 32 bytes per member. The per-member results are those of zultra_hip_inflate_members(..., ZULTRA_FLAG_GZIP_FRAMING, the index's items, ...), field
 * for field: a member whose ISIZE lies is 13 (too low) or 16 (too high). results (host, results_cap entries) may be NULL. Returns the number of indexed
 * members whose reason is not 0; -1 for bad arguments (src / dst / res NULL, src_size 0, a bad device), HIP errors and stop 4 (res filled). A stop of 1..3 is
 * no error of this call: the indexed prefix is decoded and res->src_used says where the rest begins. *_on_device as for zultra_hip_inflate_streams (of a host
 * dst only the out_size bytes of every member are written). kernel_ms (may be NULL): four — index, frame, inflate, check.
 */
typedef struct zultra_hip_index_result_s {
   uint32_t members, stop;          /* stop kinds 0..3 above; 4 = more members than `cap` / more output than dst_size (nothing decoded) */
   uint64_t out_size, src_used;     /* sum of ISIZE of the indexed members; the stop position */
   uint32_t tiles, tiles_rewalked;  /* diagnostics: tiles the chain entered, and those whose guess was not the chain's entry */
} zultra_hip_index_result_t;
int zultra_hip_index_members(int device, const void *src, size_t src_size, int src_on_device,
                             zultra_hip_inflate_item_t *items, uint32_t cap, zultra_hip_index_result_t *res, float *kernel_ms /* may be NULL */);
int zultra_hip_inflate_file(int device, const void *src, size_t src_size, int src_on_device, void *dst, size_t dst_size, int dst_on_device,
                            zultra_hip_index_result_t *res, zultra_hip_member_result_t *results /* host, results_cap; may be NULL */, uint32_t results_cap,
                            float *kernel_ms /* [4]: index, frame, inflate, check; may be NULL */);

/*
 * A BYTE RANGE of such a file: only the members that cover it are inflated. U is the concatenation of the outputs of the indexed members (the
 * chain above from p = 0, with any stop kind), F = |U| the sum of their ISIZEs. The range is clipped to U: lo = min(first, F), hi = min(first + nbytes, F), the
 * sum saturating at 2^64 - 1; out_size = hi - lo and dst[0 .. out_size) = U[lo .. hi). With out_size == 0 (nbytes == 0, or first >= F) nothing is decoded,
 * range_members is 0 and the call returns 0. Otherwise m0 is the member with ISIZE > 0 that holds byte lo and m1 the one that holds byte hi - 1; the call
 * decodes members m0 .. m1 and no others — empty members between them go through as zero-length items, as in zultra_hip_inflate_file —, results[k] is what
 * zultra_hip_inflate_file reports for member m0 + k, field for field, and the return value is the number of decoded members whose reason is not 0. A member
 * outside m0 .. m1 is never looked at beyond what the index reads: if it is damaged the call does not notice. A stop of 1..3 is no error: res->stop reports it
 * and the range is served from the indexed prefix. If out_size > dst_size, or results != NULL and range_members > results_cap, stop is 4, the call returns -1,
 * nothing is written and res says how much room is needed. Bad arguments (-1) are those of zultra_hip_inflate_file.
 * Members that lie wholly inside [lo, hi) are decoded straight into their place in dst, also where dst is a device pointer used in place; the one or two that
 * straddle an end of the range are decoded and CRC-checked in full in memory the call owns, and their slices moved into dst. Nothing outside
 * dst[0 .. out_size) is ever written (of a host dst only out_size bytes). If a member fails, its own part of the range is unspecified and every other member's
 * bytes are in place. The call owns memory in proportion to the tile count, the members decoded and the straddling members' ISIZEs, never to F or to the
 * file's member count, and reads back 32 bytes per decoded member.
 *   members, stop, src_used, tiles, tiles_rewalked : the index of the WHOLE source, as in zultra_hip_index_result_t; file_size is F
 *   first_member, range_members : m0 and m1 - m0 + 1
 * kernel_ms (may be NULL): five — index, select + items, frame, inflate, check + edges.
 */
typedef struct zultra_hip_range_result_s {
   uint32_t members, stop;                 /* the index of the whole source; 4 = too little room (nothing decoded) */
   uint64_t file_size, src_used;           /* sum of ISIZE of the indexed members; the stop position */
   uint32_t first_member, range_members;   /* the members decoded: first_member .. first_member + range_members - 1 */
   uint64_t out_size;                      /* bytes of the range that exist: what was (or would be) written to dst[0 .. out_size) */
   uint32_t tiles, tiles_rewalked;
} zultra_hip_range_result_t;
int zultra_hip_inflate_range(int device, const void *src, size_t src_size, int src_on_device, uint64_t first, uint64_t nbytes,
                             void *dst, size_t dst_size, int dst_on_device, zultra_hip_range_result_t *res,
                             zultra_hip_member_result_t *results /* host, results_cap; may be NULL */, uint32_t results_cap,
                             float *kernel_ms /* [5]: index, select + items, frame, inflate, check + edges; may be NULL */);

/*
 * Many small independent inputs ("files", BASELINE.json configuration 5: 4 KiB records, each its own stream). A files
 * context takes inputs below 8192 bytes — the splitter never cuts those (blockdeflate.c:646), so a batch needs no host
 * decision and its whole kernel sequence is replayed from one captured hipGraph. zultra_hip_compress_files runs
 * stages 1-3 with every input as a max-block without history, then lays the raw deflate streams end to end in the
 * device stream buffer (zultra_hip_stream_read): input i occupies bytes file_off[i] .. file_off[i+1]. Each equals what
 * zultra_memory_compress(input i, ZULTRA_FLAG_RAW_DEFLATE) produces; zultra_hip_frame_members (below) lays the same
 * streams out as complete gzip, zlib or BGZF members. zultra_hip_stitch_files does the assembly alone for a
 * batch already compressed with zultra_hip_compress_blocks. Returns the number of inputs, or a negative error.
 */
zultra_hip_ctx_t *zultra_hip_create_files(int device, uint32_t max_file_size, uint32_t max_files);
int zultra_hip_compress_files(zultra_hip_ctx_t *ctx, const void *data, size_t data_size, int data_on_device, const uint64_t *offsets,
                              const uint32_t *sizes, uint32_t nfiles, uint64_t *file_off /* nfiles + 1 */);
int zultra_hip_stitch_files(zultra_hip_ctx_t *ctx, uint64_t *file_off /* blocks + 1 */);

/*
 * Framed members: every max-block of the last batch of ANY context becomes one complete member in the context's stream buffer
 * (zultra_hip_stream_device / zultra_hip_stream_read), the members back to back: header, the max-block's raw deflate stream exactly as
 * zultra_hip_stitch_files lays it out (BFINAL on its last sub-block, padded to a byte), trailer. The device writes all of it — the assembly leaves room
 * around every stream, a kernel behind the bit mover fills the room and finalises the checksums from the per-max-block parts —, so a batch of members
 * reaches the host in one read, or goes straight into zultra_hip_inflate_members / zultra_hip_inflate_file without leaving the device.
 *   framing  : 0 raw (zultra_hip_stitch_files with the offsets as {off, size}; check = 0), ZULTRA_FLAG_ZLIB_FRAMING, ZULTRA_FLAG_GZIP_FRAMING
 *              (libzultra.h) — member b is then zultra_memory_compress(max-block b, framing, max_block >= n) byte for byte: the header of
 *              zultra_frame_encode_header without a dictionary, the trailer of zultra_frame_encode_footer —, or ZULTRA_HIP_FRAME_BGZF: the header
 *              1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 + BSIZE (member size - 1, u16 LE), the trailer CRC-32 + ISIZE. Anything else is -1
 *   bgzf_eof : BGZF only: != 0 puts BGZF's 28-byte empty member behind the last one (the end of a file)
 *   members  : host, one per max-block: first byte and size of the member in the stream buffer, the CRC-32 / Adler-32 as written, flags bit 0 =
 *              oversize (BGZF: n > 65536 or a member above 65536 bytes)
 *   total_bytes : the members and the end marker
 * Every max-block must stand alone (prev == 0), else -1. Returns 0; -1 for bad arguments, no batch, and HIP errors; -2 where the reference fails with
 * ZULTRA_ERROR_DST or the members do not fit the stream buffer; -3 (BGZF) where a member is oversize — members[] is filled, flags set. Nothing is written
 * for -2 and -3. A context of max-blocks of at most ZULTRA_HIP_BGZF_BLOCK bytes never returns -3: the per-max-block buffer bound keeps every stream
 * short enough. zultra_hip_verify_device afterwards verifies the framed buffer; zultra_hip_stitch_files afterwards assembles the
 * plain layout again.
 */
#define ZULTRA_HIP_FRAME_BGZF 4u   /* next to 0 raw, ZULTRA_FLAG_ZLIB_FRAMING 1, ZULTRA_FLAG_GZIP_FRAMING 2 */
#define ZULTRA_HIP_BGZF_BLOCK 65280u   /* bgzip's block size: input bytes per BGZF member */
typedef struct zultra_hip_member_s { uint64_t off, size; uint32_t check, flags; } zultra_hip_member_t;  /* flags bit 0: oversize (BGZF) */
int zultra_hip_frame_members(zultra_hip_ctx_t *ctx, unsigned int framing, int bgzf_eof,
                             zultra_hip_member_t *members /* host, blocks */, uint64_t *total_bytes);
/* A measurement hook (tools/frame_time.py), no part of the framing itself: device time of the last zultra_hip_frame_members' launches, milliseconds, from
 * HIP events on the context's stream — the scan with the clearing behind it, the bit mover, the frame kernel. */
void zultra_hip_last_frame_ms(const zultra_hip_ctx_t *ctx, float *ms /* [3] */);

/*
 * A ZIP archive's entries: the max-blocks of the last batch of ANY context as entries of a ZIP archive, written on the device into a
 * second, context-owned buffer (zultra_hip_zip_device / zultra_hip_zip_read) — a gather behind the plain files-form assembly. The buffer holds the LOCAL
 * PART, per entry {30-byte local header, name, the raw deflate stream exactly as zultra_hip_stitch_files lays it out}, and behind it at a 16-byte aligned
 * position (central_at) the CENTRAL PART, per entry {46-byte central header, name}. An archive is the local parts of its batches, their central parts,
 * and the end records of zultra_zip_end_records (libzultra.h).
 *   names, name_off : entry i is named names + name_off[i] .. name_off[i + 1], 1 .. 65535 bytes of UTF-8 (general purpose flag 0x0800 is set)
 *   entry_block     : the max-block of entry i, or 0xFFFFFFFF for an EMPTY entry — a zero-length file or a directory: method 0, sizes 0, CRC 0, version
 *                     needed 10. The max-blocks named are every max-block of the batch, once each, in increasing order. NULL: entry i is max-block i, n of them
 *   base_off        : where this local part will stand in the archive: what the central headers' offsets and entries[].local_off count from
 *   dos_datetime    : date << 16 | time for every entry; 0 = 1980-01-01 00:00:00 (0x00210000)
 *   entries         : host, n, may be NULL: offset of the local header, sizes, CRC-32 and name length as written (as found where the call fails)
 * Other entries are method 8, version needed 20; no extra fields, no comments, attributes 0. The stream buffer must hold the plain files form of the batch:
 * a files context's batch brings it, zultra_hip_stitch_files makes it; where it is absent (no assembly yet, framed members since) the call runs that assembly
 * first. Otherwise the stream buffer is not written: zultra_hip_verify_device, zultra_hip_stitch_files and zultra_hip_frame_members behave as before the call.
 * Returns 0; -1 for bad arguments (no batch, a max-block with history, a name of length 0 or above 65535, an entry_block that is not the batch's max-blocks
 * once each in increasing order) and HIP errors; -2 where the assembly fails as zultra_hip_stitch_files does, or base_off + local_bytes + central_bytes reaches
 * 0xFFFFFFFF (sizes and offsets from there on need ZIP64 fields per entry, which are not written). A refused call writes nothing.
 */
typedef struct zultra_hip_zip_entry_s { uint64_t local_off; uint32_t comp_size, size, crc32, name_len; } zultra_hip_zip_entry_t;
int zultra_hip_zip_members(zultra_hip_ctx_t *ctx, const void *names, const uint32_t *name_off /* n + 1, host */,
                           const uint32_t *entry_block /* n, host; NULL: entry i = max-block i */, uint32_t n,
                           uint64_t base_off, uint32_t dos_datetime /* date << 16 | time; 0 = 1980-01-01 00:00:00, i.e. 0x00210000 */,
                           zultra_hip_zip_entry_t *entries /* host, n; may be NULL */, uint64_t *local_bytes, uint64_t *central_bytes);
const void *zultra_hip_zip_device(const zultra_hip_ctx_t *ctx, uint64_t *central_at);   /* the buffer; where the central part starts in it */
int zultra_hip_zip_read(zultra_hip_ctx_t *ctx, void *out, size_t offset, size_t nbytes);
/* A measurement hook (tools/zip_time.py): device time of the last zultra_hip_zip_members' launches, milliseconds. */
void zultra_hip_last_zip_ms(const zultra_hip_ctx_t *ctx, float *ms /* [3]: scan, records, copy */);

/*
 * Streams of several max-blocks in one batch: the GROUPED assembly. A grouping of the last batch is stream_first[0 .. nstreams), host, max-block
 * indices: stream_first[0] == 0, strictly increasing, below the batch's block count; stream s is max-blocks stream_first[s] .. stream_first[s + 1] - 1, the last
 * stream runs to the end of the batch. It is valid only if the first max-block of every stream has prev == 0 and every other max-block b continues b - 1:
 * win_off[b] + prev[b] == win_off[b-1] + prev[b-1] + n[b-1], prev[b] == min(32768, the stream's bytes in front of b), and n[b-1] == the context's max-block size.
 * Under these rules stream s is BYTE FOR BYTE what zultra_memory_compress(input s, framing, the context's max-block size) produces: inside a stream the bit phase
 * is carried from max-block to max-block and the history is real, between streams there is a BFINAL and a byte-aligned restart. Anything else returns -1 and
 * nothing is written. Explicit assembly only: nothing of it goes out with a batch (no zultra_hip_stitch_with_batch, no captured graph), and after it
 * zultra_hip_stitch_files, zultra_hip_stitch_device, zultra_hip_frame_members and zultra_hip_zip_members behave as after any other explicit assembly;
 * zultra_hip_verify_device verifies it.
 * zultra_hip_frame_streams: the streams as members back to back in the stream buffer.
 *   framing  : 0 (raw deflate streams back to back), ZULTRA_FLAG_ZLIB_FRAMING or ZULTRA_FLAG_GZIP_FRAMING; BGZF is -1 — a BGZF member cannot hold several max-blocks
 *   members  : host, nstreams: off, size, check = the stream's Adler-32 / CRC-32 (0 for raw), flags = 0. gzip's ISIZE is the stream's size
 * Returns as zultra_hip_frame_members: 0; -1 for bad arguments, an invalid grouping, no batch, HIP errors; -2 where the reference fails with ZULTRA_ERROR_DST, the
 * members do not fit the stream buffer, or a stream reaches 2^32 bytes. Nothing is written for -1 and -2.
 * zultra_hip_zip_streams: zultra_hip_zip_members with the streams as entries — entry_stream[i] is the stream of entry i or 0xFFFFFFFF for an empty entry, the streams
 * named are every stream of the grouping once, in increasing order (NULL: entry i is stream i); names, name_off, base_off, dos_datetime, entries, local_bytes,
 * central_bytes, the 0xFFFFFFFF limit and the return codes are zultra_hip_zip_members'. It gathers from the plain grouped form (framing 0) where the stream buffer
 * holds it FOR THE SAME GROUPING, and assembles it first otherwise.
 */
int zultra_hip_frame_streams(zultra_hip_ctx_t *ctx, const uint32_t *stream_first /* host, nstreams */, uint32_t nstreams, unsigned int framing,
                             zultra_hip_member_t *members /* host, nstreams */, uint64_t *total_bytes);
int zultra_hip_zip_streams(zultra_hip_ctx_t *ctx, const uint32_t *stream_first /* host, nstreams */, uint32_t nstreams, const void *names, const uint32_t *name_off /* n + 1, host */,
                           const uint32_t *entry_stream /* n, host; NULL: entry i = stream i */, uint32_t n, uint64_t base_off, uint32_t dos_datetime,
                           zultra_hip_zip_entry_t *entries /* host, n; may be NULL */, uint64_t *local_bytes, uint64_t *central_bytes);
/* A measurement hook (tools/streams_time.py): device time of the last grouped assembly's launches, milliseconds. */
void zultra_hip_last_streams_ms(const zultra_hip_ctx_t *ctx, float *ms /* [3]: scan, fold, frame kernel */);
/* Diagnostics (tests): the items of the last assembly's scan, per sub-block {u64 dst_bit, u32 stored, u32 is_final} — returns their count, -1 on errors —; and what the
 * host's serial statement of the grouped rule gives for a grouping of the last batch: the same items (nsubs; may be NULL), file_off (nstreams + 1; may be NULL) and
 * *end_bit. 0; -1 for an invalid grouping or framing; -2 where the reference fails with ZULTRA_ERROR_DST or a stream reaches 2^32 bytes. */
int zultra_hip_stitch_items(zultra_hip_ctx_t *ctx, void *items /* nsubs x 16 bytes */);
int zultra_hip_plan_streams(zultra_hip_ctx_t *ctx, const uint32_t *stream_first, uint32_t nstreams, unsigned int framing, void *items, uint64_t *file_off, uint64_t *end_bit);

/*
 * A ZIP archive READ: the central directory indexed on the device, then every entry checked against its local header, inflated or copied,
 * and its CRC-32 taken and compared there. The caller names the directory — src[central_at .. central_at + central_size), from zultra_zip_find_end
 * (libzultra.h) or from zultra_hip_zip_device —, the device finds the records: one starts at p when 46 bytes lie in front of the directory's end, src[p..p+4) =
 * 50 4b 01 02 and, with n, m, k the le16 values at p + 28, p + 30, p + 32, p + 46 + n + m + k does not pass the directory's end; the next is behind it. The
 * chain from central_at is walked in tiles of ZULTRA_HIP_INDEX_TILE bytes (default here: 16 KiB) as zultra_hip_index_members walks a gzip file, and equals the serial walk bit for bit.
 *   dirent         : central_at (the record's position in src; the name lies at central_at + 46), local_off as the record names it, dst_off = the 64-bit
 *                    sum of the `size` fields of the records in front, whatever becomes of those entries, and the record's fields
 *   stop           : why the chain ended at central_at + dir_used — 0 the directory's end; 1 fewer than 46 bytes left, or no signature; 2 a record that runs
 *                    past the end; and 4 = more entries than `cap`, or (zultra_hip_unzip) more output than dst_size: nothing was written, entries / out_size say
 *                    how much room the archive needs. out_size is known before a byte is inflated: an archive cannot make the call write more than dst_size
 *   tiles, tiles_rewalked : as for zultra_hip_index_members
 * zultra_hip_zip_index: the index alone. dirents (host, cap) may be NULL with cap 0 to learn the counts. Returns 0; -1 for bad arguments (src NULL, src_size 0,
 * a directory outside src, a bad device, dirents NULL with cap > 0), HIP errors and stop 4 (res filled, nothing written). kernel_ms: the index kernels.
 * zultra_hip_unzip: entry i goes to dst + dirent[i].dst_off. local_delta: what is added to a record's local_off to find the local header in src — the size of
 * whatever stands in front of the archive (a self-extractor's stub) for a file, -base_off for a local part standing in zultra_hip_zip_device. An entry's reason,
 * in this order:
 *   17 decided from the dirent alone: a method other than 0 (stored) and 8 (deflate); flag bit 0 or 6 (encrypted) or 5 (patched); comp_size, size or local_off
 *      0xFFFFFFFF (the ZIP64 extra field is not read)
 *   14 the local header: its 30 bytes do not lie in src, no 50 4b 03 04, its name (length or bytes) or its method differ from the central record's, the data
 *      runs past src, a stored entry with comp_size != size. The local header's sizes and CRC, a data descriptor (flag bit 3) and a ZIP64 extra field there are
 *      not looked at: the central record is the authority
 *   1..13 the inflate kernel's own; its room is `size`, so more output than that is 13
 *   16 out_size != size, then 15 the CRC-32 of the output differs from the record's (16 first, unlike gzip: a short output fails both, and 16 says more)
 * results[i]: blocks, out_size as the inflate kernel left them (a stored entry: 0 and size); src_used the deflate bytes consumed (stored: comp_size), which a
 * caller compares with comp_size; head_size = 30 + the local name and extra lengths; check the CRC-32 COMPUTED, whenever bytes were summed. dirents and results
 * (host, cap entries each) may be NULL. Returns the number of entries whose reason is not 0; -1 for bad arguments, HIP errors, stop 4, and a stop of 1 or 2 —
 * nothing is decoded from a directory that does not end where it should. src, dst, *_on_device as for zultra_hip_inflate_streams (of a host dst only the bytes
 * entries wrote come back). kernel_ms (may be NULL): five — index, local headers, inflate, copy, check.
 * Not read: ZIP64 fields per entry, encryption, methods other than 0 and 8, multi-disk archives, an archive without a central directory. One large entry
 * decodes at the speed of one wave.
 */
#define ZULTRA_HIP_UNZIP_UNSUPPORTED 17
typedef struct zultra_hip_zip_dirent_s {
   uint64_t central_at, local_off, dst_off;
   uint32_t comp_size, size, crc32, name_len;
   uint16_t method, flags, extra_len, comment_len;
} zultra_hip_zip_dirent_t;
typedef struct zultra_hip_zip_index_result_s {
   uint32_t entries, stop;          /* stop kinds 0..2 above; 4 = more entries than `cap` / more output than dst_size (nothing decoded) */
   uint64_t out_size, dir_used;     /* sum of `size` of the indexed records; bytes of the directory the chain covers */
   uint32_t tiles, tiles_rewalked;
} zultra_hip_zip_index_result_t;
int zultra_hip_zip_index(int device, const void *src, size_t src_size, int src_on_device, uint64_t central_at, uint64_t central_size,
                         zultra_hip_zip_dirent_t *dirents /* host, cap; NULL with cap 0 */, uint32_t cap, zultra_hip_zip_index_result_t *res,
                         float *kernel_ms /* may be NULL */);
int zultra_hip_unzip(int device, const void *src, size_t src_size, int src_on_device, uint64_t central_at, uint64_t central_size, int64_t local_delta,
                     void *dst, size_t dst_size, int dst_on_device, zultra_hip_zip_index_result_t *res,
                     zultra_hip_zip_dirent_t *dirents /* host, cap; may be NULL */, zultra_hip_member_result_t *results /* host, cap; may be NULL */, uint32_t cap,
                     float *kernel_ms /* [5]: index, locals, inflate, copy, check; may be NULL */);

/* CRC-32 of every max-block of the last batch, computed on the device while the blocks are compressed: out[b] is the
 * linear part (zero initial state, no final inversion). zultra_crc32_append() folds one block into a running gzip CRC
 * exactly as zultra_frame_update_checksum(crc, block, len, GZIP) would (reference src/frame.c:324-354,473-480). */
int zultra_hip_block_crc32(const zultra_hip_ctx_t *ctx, uint32_t *out);
uint32_t zultra_crc32_append(uint32_t crc, uint32_t block_linear_crc, size_t block_len);
/* Same for zlib framing: out[2b] = sum of the bytes of max-block b, out[2b+1] = sum of (n - i) * byte[i], both mod 65521.
 * zultra_adler32_append() folds one block into a running Adler-32 exactly as zultra_frame_update_checksum(adler, block,
 * len, ZLIB) would (reference src/frame.c:74-138). */
int zultra_hip_block_adler32(const zultra_hip_ctx_t *ctx, uint32_t *out);
uint32_t zultra_adler32_append(uint32_t adler, uint32_t block_sum, uint32_t block_weighted_sum, size_t block_len);
uint32_t zultra_crc32_append_many(uint32_t crc, const uint32_t *block_linear_crc, const uint32_t *block_len, uint32_t nblocks);

#ifdef __cplusplus
}
#endif
#endif /* ZULTRA_HIP_H */
