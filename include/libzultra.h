/*
 * libzultra.h — the drop-in public API of the MI355X build.
 *
 * Call-compatible with the reference's src/libzultra.h (names, argument meaning, status values, struct layout:
 * :49-61 status enum, :64-75 flags/defaults, :78-93 zultra_stream_t, :104-157 functions) and, for the helpers the
 * reference's CLI links against, with src/frame.h:65-119 and src/dictionary.h:60-67. A program written against the
 * reference relinks against libzultra_amd.so unchanged; the bytes it gets back are identical.
 *
 * Behavioural contract kept from the reference:
 *  - max-blocks are cut at exactly nMaxBlockSize bytes whatever the chunking of the calls (libzultra.c:259-269);
 *  - a full max-block is compressed only once more input is seen or ZULTRA_FINALIZE is given (:269);
 *  - ZULTRA_OK = "call again", ZULTRA_STREAM_END once after the footer is consumed, then ZULTRA_ERROR_COMPRESSION;
 *  - an empty input is never finalized (:275), so zultra_memory_compress(…, 0 bytes) returns (size_t)-1;
 *  - zultra_memory_compress returns (size_t)-1 if the output buffer cannot take the whole stream.
 * Difference in *how*: when a call hands over several max-blocks at once they are compressed as one device batch.
 * The per-block work runs on the GPU only; without a usable HIP device zultra_stream_init fails with
 * ZULTRA_ERROR_MEMORY... never with a silent CPU path.
 */
#ifndef LIBZULTRA_AMD_H
#define LIBZULTRA_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- format constants (reference src/format.h:37-50) ---- */
#define MIN_MATCH_SIZE 3
#define MAX_MATCH_SIZE 258
#define MIN_OFFSET 1
#define MAX_OFFSET 32768
#define HISTORY_SIZE 0x8000

/* ---- framing helpers (reference src/frame.h) ---- */
#define ZULTRA_HEADER_SIZE 4
#define ZULTRA_FRAME_SIZE 4
#define ZULTRA_FOOTER_SIZE 8
#define ZULTRA_ENCODE_ERR (-1)

typedef unsigned int zultra_frame_checksum_t;

int zultra_frame_get_header_size(const unsigned int nFlags, const void *pDictionaryData, const int nDictionarySize);
int zultra_frame_encode_header(unsigned char *pFrameData, const int nMaxFrameDataSize, const unsigned int nFlags,
                               const void *pDictionaryData, const int nDictionarySize);
zultra_frame_checksum_t zultra_frame_init_checksum(const unsigned int nFlags);
zultra_frame_checksum_t zultra_frame_update_checksum(zultra_frame_checksum_t nChecksum, const void *pData, size_t nDataSize,
                                                     const unsigned int nFlags);
int zultra_frame_get_footer_size(const unsigned int nFlags);
int zultra_frame_encode_footer(unsigned char *pFrameData, const int nMaxFrameDataSize, const zultra_frame_checksum_t nChecksum,
                               long long nOriginalSize, const unsigned int nFlags);

/* ---- status, flags ---- */
typedef enum _zultra_stream_e
#if defined(__cplusplus) && __cplusplus > 199711L
   : int
#endif
{
   ZULTRA_OK = 0,                 /* progress made; call again for more */
   ZULTRA_STREAM_END,             /* footer fully delivered */
   ZULTRA_ERROR_SRC = -1,
   ZULTRA_ERROR_DST = -2,
   ZULTRA_ERROR_DICTIONARY = -3,
   ZULTRA_ERROR_MEMORY = -4,
   ZULTRA_ERROR_COMPRESSION = -5,
} zultra_status_t;

#define ZULTRA_FLAG_DEFLATE_FRAMING 0   /* raw deflate */
#define ZULTRA_FLAG_ZLIB_FRAMING 1      /* RFC 1950 */
#define ZULTRA_FLAG_GZIP_FRAMING 2      /* RFC 1952 */

#define ZULTRA_CONTINUE 0
#define ZULTRA_FINALIZE 1

#define ZULTRA_DEFAULT_MAX_BLOCK_SIZE 1048576

/* ---- dictionary helpers (reference src/dictionary.h) ---- */
zultra_status_t zultra_dictionary_load(const char *pszDictionaryFilename, void **ppDictionaryData, int *pDictionaryDataSize);
void zultra_dictionary_free(void **ppDictionaryData);

/* ---- streaming API ---- */
typedef struct _zultra_compressor_s zultra_compressor_t;

typedef struct _zultra_stream_s {
   const unsigned char *next_in;
   size_t avail_in;
   unsigned long long total_in;

   unsigned char *next_out;
   size_t avail_out;
   unsigned long long total_out;

   void *(*zalloc)(void *opaque, unsigned int items, unsigned int size);
   void (*zfree)(void *opaque, void *address);
   void *opaque;

   zultra_compressor_t *state;
   zultra_frame_checksum_t adler;
} zultra_stream_t;

zultra_status_t zultra_stream_init(zultra_stream_t *pStream, const unsigned int nFlags, unsigned int nMaxBlockSize);
zultra_status_t zultra_stream_set_dictionary(zultra_stream_t *pStream, const void *pDictionaryData, const int nDictionaryDataSize);
zultra_status_t zultra_stream_compress(zultra_stream_t *pStream, const int nDoFinalize);
void zultra_stream_end(zultra_stream_t *pStream);

/* ---- in-memory API ---- */
size_t zultra_memory_bound(size_t nInputSize, const unsigned int nFlags, unsigned int nMaxBlockSize);
size_t zultra_memory_compress(const unsigned char *pInputData, size_t nInputSize, unsigned char *pOutBuffer,
                              size_t nMaxOutBufferSize, const unsigned int nFlags, unsigned int nMaxBlockSize);

/* ---- additions of this build (not in the reference) ---- */
/* As zultra_memory_compress with a preset dictionary (what zultra_stream_set_dictionary + one FINALIZE call do). */
size_t zultra_memory_compress_dict(const unsigned char *pInputData, size_t nInputSize, unsigned char *pOutBuffer,
                                   size_t nMaxOutBufferSize, const unsigned int nFlags, unsigned int nMaxBlockSize,
                                   const void *pDictionaryData, int nDictionaryDataSize);
/* Device the library runs on (default 0, or env ZULTRA_HIP_DEVICE); call before the first stream is created. */
void zultra_set_device(int nDevice);
/* Devices zultra_memory_compress spreads an input over (default: env ZULTRA_HIP_DEVICES="0,1,...", else the one device above). The
 * max-blocks of the input are cut into contiguous shards, one host thread and one device context per entry compress them side by
 * side, and the shards' bit strings are stitched in stream order on their own devices: the output bytes do not depend on the list.
 * An entry may repeat a device ("0,0": two contexts on device 0, the transfers of one shard next to the kernels of the other;
 * without a list ZULTRA_HIP_MEMORY_LANES=n does the same on the one device, default 1, and 0 sends the call through the stream API).
 * Returns nDevices, or -1 when an entry is not a visible device (the list is then left empty). nDevices = 0 clears the list. */
int zultra_set_devices(const int *pDevices, int nDevices);
/* zultra_stream_end frees everything the stream owns through zfree, like the reference (libzultra.c:521-565) — except that the
 * device context (device memory and pinned staging) of a finished stream is kept for the next stream of the same geometry:
 * creating one takes ~45 device allocations. zultra_release_cached_contexts() destroys the contexts kept that way (at most
 * two); with the environment variable ZULTRA_HIP_CACHE=0 none is ever kept and zultra_stream_end releases the device memory
 * itself. Returns the number of contexts destroyed. */
int zultra_release_cached_contexts(void);
/* Verification (default off; nEnable != 0 or the environment variable ZULTRA_HIP_VERIFY=1 turns it on): every batch the library stitches on a
 * device is inflated there and compared with its input before its bytes are handed out (include/zultra_hip.h: zultra_hip_verify_device) —
 * the stream API, zultra_memory_compress, zultra_memory_compress_dict, every shard of a call spread over several contexts. On a mismatch
 * zultra_stream_compress returns ZULTRA_ERROR_COMPRESSION, the memory calls return (size_t)-1, and one line with the report goes to stderr.
 * The check covers the deflate body, not the framing's header and footer. With ZULTRA_HIP_HOST_STITCH=1 the batch is stitched on the device
 * as well, for the check, at the phase the host stitcher starts from. Off, the library launches nothing and reads nothing for it. */
void zultra_set_verify(int nEnable);
/* Input bytes verified that way in this process since the library was loaded: how a caller knows the check ran over everything. */
unsigned long long zultra_verified_bytes(void);
/* Decompression (the reference has none: its tool links zlib for its own check). pIn is one complete stream in the framing nFlags names, as for
 * compression: raw deflate (the stream must end at nIn), zlib (2-byte header with the CMF / FLG check, FDICT is rejected, Adler-32 checked) or gzip
 * (RFC 1952 header with FEXTRA, FNAME, FCOMMENT and FHCRC skipped, CRC-32 and ISIZE checked). The deflate stream is inflated on the device
 * (include/zultra_hip.h: zultra_hip_inflate_streams — one stream, so at the speed of one wave), the checksum is taken on the host. Returns the
 * number of bytes written to pOut, or (size_t)-1: a bad header, a stream that does not decode, bytes behind its end, a checksum mismatch, more
 * output than nMaxOut, no device. */
size_t zultra_memory_decompress(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nMaxOut, const unsigned int nFlags);
/* ... of a stream compressed against a preset dictionary (zultra_memory_compress_dict, zultra_stream_set_dictionary, zlib's deflateSetDictionary).
 * Raw deflate and gzip: the dictionary is the history of the stream, as it was on the way in. zlib: a header with FDICT must carry the Adler-32 of
 * the WHOLE dictionary as its DICTID (what zultra_frame_encode_header writes, also for dictionaries above 32 KiB), else (size_t)-1 — a wrong
 * dictionary, or FDICT and no dictionary given; a header without FDICT ignores the dictionary, as zlib does. In every framing the last
 * min(nDictSize, 32768) bytes are what matches can reach (include/zultra_hip.h: zultra_hip_inflate_streams_dict). pDict == NULL or nDictSize <= 0:
 * no dictionary. Everything else as zultra_memory_decompress, which keeps rejecting FDICT. */
size_t zultra_memory_decompress_dict(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nMaxOut, const unsigned int nFlags,
                                     const void *pDict, int nDictSize);
/* n members of ONE framing in one call (include/zultra_hip.h: zultra_hip_inflate_members — headers, inflate, checksums and trailers on the device),
 * each complete in pIn at pInOff[i] .. + pInSize[i], decoded to pOut + pOutOff[i] (at most pOutCap[i] bytes; the ranges must not overlap);
 * pOutSize[i] = bytes written or (size_t)-1. Returns the number of members that failed, (size_t)-1 for bad arguments or no device. A member must
 * fill its range of pIn exactly (bytes behind its trailer fail it). Two differences from calling zultra_memory_decompress_dict member by member: a
 * gzip header's FHCRC is checked, and with a dictionary a zlib member WITHOUT FDICT fails (put such members into a call without one). */
size_t zultra_memory_decompress_batch(const unsigned char *pIn, size_t nIn, const size_t *pInOff, const size_t *pInSize, unsigned char *pOut, size_t nMaxOut,
                                      const size_t *pOutOff, const size_t *pOutCap, size_t *pOutSize, size_t n, const unsigned int nFlags,
                                      const void *pDict, int nDictSize);

/* gzip(1) over a whole file: pIn is any number of gzip members back to back — what bgzip, pigz -i or `cat a.gz b.gz` write — and pOut receives the
 * concatenation of their outputs. The source is uploaded once. Runs of BGZF members (a `BC` extra subfield with the member's size: include/zultra_hip.h,
 * zultra_hip_inflate_file) are found and inflated on the device in one batch each; a member without that hint is decoded on its own, at the speed of
 * one wave, and the walk goes on behind it. *pnMembers (may be NULL) = the members decoded. Returns the bytes written, or (size_t)-1: a member that
 * failed (header, stream, CRC-32, ISIZE), bytes behind the last member that are no member (trailing garbage, trailing zeros, a member cut off), more
 * output than nMaxOut, an empty input, no device. A gzip header's FHCRC is checked, as in zultra_memory_decompress_batch (zultra_memory_decompress
 * skips the two bytes). No dictionary. */
size_t zultra_memory_decompress_members(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nMaxOut, size_t *pnMembers /* may be NULL */);

/* A byte range of a BGZF file, and bgzip's `.gzi` index of one (include/zultra_hip.h: zultra_hip_inflate_range).
 * The index: le64 N, then N pairs le64 compressed offset, le64 uncompressed offset, each pair the start of a member. zultra_memory_index_gzi writes one pair
 * for every indexed member of pIn but the first, in order, empty members included (byte equality with bgzip's own file is not claimed; the reader below takes
 * any list of member starts, as bgzip's are). It succeeds only where the whole input is a chain of BGZF members (stop kind 0). pGzi == NULL returns the size
 * needed. Returns the bytes written, or (size_t)-1: any other stop, nMaxGzi too small, bad arguments, no device.
 * zultra_memory_decompress_range writes bytes [nFirst, nFirst + nBytes) of the concatenated output to pOut and returns their count: short at the end of the
 * file, 0 behind it. Only the members that hold those bytes are inflated and checked. Without an index (pGzi NULL) the whole input is uploaded and indexed on
 * the device; (size_t)-1 if a decoded member fails, the range exceeds nMaxOut, or the index stops with kind 1..3 and nFirst + nBytes reaches past the indexed
 * prefix (the call cannot know what follows). With an index, only the window pIn[c0 .. c1) is uploaded: (c0, u0) the last pair with u <= nFirst — (0, 0) in
 * front of the first —, (c1, u1) the first pair with u >= nFirst + nBytes, c1 the end of the input without one; bytes of pIn outside the window are never
 * read. The index is validated — nGzi == 8 + 16 N, compressed offsets strictly increasing, above 0 and below nIn, uncompressed offsets not decreasing — and so
 * is what it says of the window: a member starts at the window's byte 0, the chain ends exactly at c1, and where c1 came from a pair the window's output is
 * u1 - u0 bytes. Anything else is (size_t)-1, an index that lies included. */
size_t zultra_memory_index_gzi(const unsigned char *pIn, size_t nIn, unsigned char *pGzi /* may be NULL */, size_t nMaxGzi);
size_t zultra_memory_decompress_range(const unsigned char *pIn, size_t nIn, unsigned long long nFirst, size_t nBytes,
                                      unsigned char *pOut, size_t nMaxOut, const unsigned char *pGzi /* may be NULL */, size_t nGzi);

/* bgzip(1): pIn cut into blocks of nBlockSize bytes (0 = 65280, bgzip's; at most 65280; the last block is shorter), every block an independent BGZF
 * member — a gzip member whose `BC` extra subfield holds its size, at most 65536 bytes —, and BGZF's 28-byte empty member behind the last: the container
 * zultra_memory_decompress_members and zultra_hip_inflate_file read in parallel. The blocks are compressed as max-blocks without history, in as many
 * device batches as the context's capacity needs; headers, CRC-32 and ISIZE are written on the device (include/zultra_hip.h: zultra_hip_frame_members)
 * and every batch's framed bytes are read back once. A member's deflate stream is zultra_memory_compress(block, ZULTRA_FLAG_RAW_DEFLATE, nBlockSize)'s.
 * An empty input gives the 28-byte marker alone. Returns the bytes written, or (size_t)-1: nMaxOut too small (zultra_memory_bound_bgzf is enough),
 * nBlockSize above 65280, a device failure, no device. One device (zultra_set_device); with zultra_set_verify every batch is verified after framing. */
size_t zultra_memory_bound_bgzf(size_t nIn, unsigned int nBlockSize);
size_t zultra_memory_compress_bgzf(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nMaxOut, unsigned int nBlockSize /* 0 = 65280; at most 65280 */);
/* The writing counterpart of zultra_memory_decompress_batch: n independent inputs, pIn + pInOff[i] .. + pInSize[i], give n members of ONE framing
 * (nFlags: raw deflate, zlib or gzip) back to back in pOut, member i at pOutOff[i] .. pOutOff[i + 1] — byte for byte what zultra_memory_compress(input i,
 * nFlags, a max-block size >= its size) returns. Inputs below 8192 bytes go through a files context (include/zultra_hip.h), larger ones through a
 * context of max-blocks; an input is ONE max-block, so at most 2 MiB. Returns the bytes written, or (size_t)-1: bad arguments, an empty input (as
 * zultra_memory_compress refuses it), an input above 2 MiB, nMaxOut too small, a device failure, no device. One device; verified like the call above. */
size_t zultra_memory_compress_batch(const unsigned char *pIn, size_t nIn, const size_t *pInOff, const size_t *pInSize, size_t n,
                                    unsigned char *pOut, size_t nMaxOut, size_t *pOutOff /* n + 1, written */, const unsigned int nFlags /* 0, ZLIB, GZIP */);

/* A complete ZIP archive of n named inputs: input i, pIn + pInOff[i] .. + pInSize[i], is the entry named pNames + pNameOff[i] .. pNameOff[i + 1] (1 .. 65535
 * bytes of UTF-8, given as they are). The inputs are grouped into device batches exactly as zultra_memory_compress_batch groups them; local headers, names,
 * streams and central directory records are laid out on the device (include/zultra_hip.h: zultra_hip_zip_members), a batch's local part is read to its place in
 * pOut, the central parts follow the last batch, then the end records. Entry i's data is byte for byte zultra_memory_compress(input i,
 * ZULTRA_FLAG_DEFLATE_FRAMING, a max-block size >= its size): method 8 always, also where stored would be a few bytes shorter. An input of size 0 is an EMPTY
 * entry — a zero-length file, or a directory where its name ends in '/': method 0 — and is not refused. nDosDateTime: date << 16 | time for every entry,
 * 0 = 1980-01-01 00:00:00. No extra fields, comments or attributes: the archive is a function of its inputs. Returns the bytes written, or (size_t)-1: bad
 * arguments, an input above 2 MiB (ONE max-block), a name of 0 or above 65535 bytes, nMaxOut too small (zultra_memory_bound_zip is enough), an archive that
 * reaches 0xFFFFFFFF bytes (ZIP64 fields per entry are not written), a device failure, no device. One device; with zultra_set_verify every batch is verified. */
size_t zultra_memory_bound_zip(size_t nInTotal, size_t nNamesTotal, size_t n);
size_t zultra_memory_compress_zip(const unsigned char *pIn, size_t nIn, const size_t *pInOff, const size_t *pInSize,
                                  const char *pNames, const size_t *pNameOff /* n + 1 */, size_t n,
                                  unsigned char *pOut, size_t nMaxOut, unsigned int nDosDateTime);
/* The same two calls for inputs of ANY size: an input is a run of max-blocks of nMaxBlockSize bytes (clamped like zultra_memory_compress's: 0 = 1 MiB, then
 * 32768 .. 2 MiB) that carries its bit phase and its history from max-block to max-block, and many such streams share a device batch (include/zultra_hip.h: the
 * grouped assembly, zultra_hip_frame_streams / zultra_hip_zip_streams). Member i — entry i's data — is byte for byte zultra_memory_compress(input i, nFlags,
 * nMaxBlockSize), for any input size. The inputs are gathered into pinned staging one behind the other; a stream lies wholly in one batch, and there are as many
 * batches as the context's max-blocks (ZULTRA_HIP_BATCH_BLOCKS) and data capacity need. LIMIT: an input with more max-blocks than one context holds is
 * refused — zultra_memory_compress remains the call for one huge input. zultra_memory_compress_streams refuses an empty input, zultra_memory_compress_zip_streams
 * makes it an empty entry. nMaxOut: the sum of zultra_memory_bound(size i, nFlags, nMaxBlockSize) suffices; for the archive (nFlags 0) add both copies of the
 * names, 76 bytes per entry, and 98. Everything else — arguments, pOutOff, names, nDosDateTime, the 0xFFFFFFFF limit of an archive, (size_t)-1, one device, the
 * verification of every batch after framing with zultra_set_verify — is as for the two calls above. */
size_t zultra_memory_compress_streams(const unsigned char *pIn, size_t nIn, const size_t *pInOff, const size_t *pInSize, size_t n,
                                      unsigned char *pOut, size_t nMaxOut, size_t *pOutOff /* n + 1, written */, const unsigned int nFlags /* 0, ZLIB, GZIP */,
                                      unsigned int nMaxBlockSize);
size_t zultra_memory_compress_zip_streams(const unsigned char *pIn, size_t nIn, const size_t *pInOff, const size_t *pInSize,
                                          const char *pNames, const size_t *pNameOff /* n + 1 */, size_t n,
                                          unsigned char *pOut, size_t nMaxOut, unsigned int nDosDateTime, unsigned int nMaxBlockSize);
/* The end of a ZIP archive, for callers who assemble one from the device layer's parts: the end of central directory record (22 bytes), and in front of it, with
 * more than 65535 entries, the ZIP64 end record and its locator (98 bytes in all). Pure host code. Returns the bytes written, or (size_t)-1: nMaxOut too small,
 * or nCentralOff or nCentralSize at or above 0xFFFFFFFF. */
size_t zultra_zip_end_records(unsigned char *pOut, size_t nMaxOut, unsigned long long nEntries, unsigned long long nCentralOff, unsigned long long nCentralSize);

/* The reading counterpart: where an archive of nArchiveSize bytes keeps its central directory, from its last nTail bytes (65535 + 22 + 20 + 56 of them hold
 * every end record there can be; fewer are fine where the archive is shorter). Pure host code. The end record is the LAST position p with 50 4b 05 06 whose
 * comment length reaches the archive's end exactly (a signature inside the archive comment is passed over). Where the 20 bytes in front of it are a ZIP64 locator
 * (50 4b 06 07, disk 0, one disk in all) the values come from the ZIP64 end record (50 4b 06 06) it points to — looked for at the offset the locator names and,
 * for an archive behind a prefix, directly in front of the locator —, which must lie inside the tail. nPrefix = the position of the end record (the ZIP64 one
 * where there is one) - nCentralSize - nCentralOff: the bytes in front of the archive proper, a self-extractor's stub, which Python's zipfile reads too; the
 * directory starts at nPrefix + nCentralOff and a local header at nPrefix + its offset. Returns 0, or -1: no end record, a disk number other than 0, a size or
 * an offset of 0xFFFFFFFF without a locator, a locator without its record, a negative prefix. An entry count of 0xFFFF without a locator is 65535 entries: what
 * zultra_zip_end_records and zipfile write for exactly that many. */
typedef struct zultra_zip_end_s {
   unsigned long long nEntries, nCentralOff, nCentralSize, nPrefix;
   int nZip64;
} zultra_zip_end_t;
int zultra_zip_find_end(const unsigned char *pTail, size_t nTail, unsigned long long nArchiveSize, zultra_zip_end_t *pEnd);

/* unzip(1) in memory: pIn is a whole ZIP archive — this library's, zip(1)'s, Python's zipfile's —, entry i is decoded to pOut + pInfo[i].nOutOff, the entries
 * back to back in the central directory's order. zultra_zip_find_end, one upload, then the directory index, the local headers, inflate / copy and the CRC-32
 * checks on the device (include/zultra_hip.h: zultra_hip_unzip, with its reasons as nStatus). pInfo[i].nNameAt: where the entry's name (nNameLen bytes, as
 * stored) lies in pIn. pOut == NULL with nMaxOut == 0 LISTS only: the directory index and the infos, returning the size the output needs. *pnEntries (may be
 * NULL) = the directory's entries. Returns the bytes written, or (size_t)-1: no end records or a directory that does not end where they say, any entry with a
 * reason, a deflated entry whose stream does not fill its comp_size, an entry count that differs from the end record's, more entries than nMaxInfo, more output
 * than nMaxOut (known before a byte is decoded), no device. pInfo is filled as far as it is known. Stored and deflated entries only; no ZIP64 fields per entry,
 * no encryption, one disk. */
typedef struct zultra_zip_info_s {
   unsigned long long nNameAt;
   unsigned int nNameLen, nMethod, nFlags, nCrc32, nCompSize, nSize;
   unsigned long long nOutOff;
   unsigned int nStatus;   /* 0, or the reason of zultra_hip_unzip */
} zultra_zip_info_t;
size_t zultra_memory_decompress_zip(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nMaxOut, zultra_zip_info_t *pInfo, size_t nMaxInfo, size_t *pnEntries /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* LIBZULTRA_AMD_H */
