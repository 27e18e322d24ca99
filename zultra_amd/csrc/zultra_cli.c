/* zultra_cli.c — command-line compressor on top of libzultra_amd.so (include/libzultra.h).
 *
 * Mirrors the compress path of the reference's tool (tool/zultra.c:97-237: open, zultra_stream_init, feed, drain, finalize)
 * with the two things that path cannot do: it takes the max-block size (-b; the reference fixes it at the
 * 1 MiB default, tool/zultra.c:151) and it feeds the stream in MiB-sized chunks instead of 16 KiB ones (tool/zultra.c:98,161),
 * so that the device sees batches of many max-blocks. The bytes written are those of the reference for the same flags and
 * block size.
 *
 *    zultra_amd_cli [-b <max block size>] [-f gzip|zlib|raw] [-k <chunk KiB>] [-d <device>] [-D <dictionary>] [-c] [-v] <infile> <outfile>
 *    zultra_amd_cli -x [-f gzip|zlib|raw] [-d <device>] [-D <dictionary>] [-v] <infile> <outfile>
 *    zultra_amd_cli -x -m [-f gzip] [-d <device>] [-v] <infile> <outfile>
 *    zultra_amd_cli -x -m -r <first>:<length> [-i <file.gzi>] [-f gzip] [-d <device>] [-v] <infile> <outfile>
 *    zultra_amd_cli -f bgzf [-b <block size>] [-i <file.gzi>] [-d <device>] [-c] [-v] <infile> <outfile>
 *    zultra_amd_cli -a <archive.zip> [-b <max block size>] [-d <device>] [-c] [-v] <file>...
 *    zultra_amd_cli -x -a <archive.zip> [-d <device>] [-v] <outdir>
 *
 * -x -a: unzip(1) — the archive (this tool's, zip(1)'s, Python's zipfile's: stored and deflated entries) is listed, then decoded on the device
 *     (zultra_memory_decompress_zip: directory index, local headers, inflate / copy and the CRC-32 checks), and every entry written under <outdir>, directories
 *     made as needed; an entry whose name ends in '/' is a directory. Before anything is written the whole archive is refused where a name is empty or absolute
 *     or holds a ".." component, a backslash or a NUL byte. With -v one line per entry, and the entries, the index's tiles and the tiles walked again.
 * -a: a ZIP archive of the files named, every file an entry under its name as given, headers and central directory written on the device
 *     (zultra_memory_compress_zip). A file is one max-block: at most 2 MiB; an empty file is an empty entry. No dictionary.
 *     With -b <max block size> a file is a stream of max-blocks of that size (zultra_memory_compress_zip_streams): files of any size that fit a device batch.
 * -f bgzf: bgzip(1) — <infile> in blocks of -b bytes (default and at most 65280), every block a BGZF member written on the device, and BGZF's end marker
 *     (zultra_memory_compress_bgzf); `-x -m -f gzip` is the way back. No dictionary: a member stands alone.
 * -r: with -x -m — only bytes <first> .. <first> + <length> of the concatenated output are written, and only the members that hold them are inflated
 *     (zultra_memory_decompress_range); a range that reaches past the end of the file is cut there. With -i the .gzi index of the file is read and only the
 *     compressed window the range needs is uploaded; the index is checked against what the window holds. With -v the first member decoded, their number and
 *     the index's tiles are printed, from a query over the whole file (zultra_hip_inflate_range without room: nothing is decoded for it).
 * -i: with -f bgzf — bgzip's .gzi index of the file written (zultra_memory_index_gzi over the output: one more index pass on the device): le64 N, then a pair
 *     of le64 compressed offset, le64 uncompressed offset for every member but the first.
 * -D: a preset dictionary, loaded as the reference's tool loads it (zultra_dictionary_load: the last 32 KiB of the file; tool/zultra.c -D). Compressing,
 *     it is set before the first zultra_stream_compress (zultra_stream_set_dictionary: the history of the first max-block; a zlib header gets FDICT and
 *     the DICTID); with -x the stream is inflated against it (zultra_memory_decompress_dict: a zlib stream's DICTID must be this dictionary's).
 * -c: every batch is inflated on the device and compared with its input before its bytes are written (zultra_set_verify); a mismatch ends the
 *     run with a non-zero status. With -v the number of bytes checked is printed.
 * -x: extract — <infile> is one stream in the framing -f names, inflated on the device (zultra_memory_decompress: header, checksum and the end of
 *     the stream are checked); a stream that does not decode ends the run with a non-zero status and an empty <outfile>.
 * -m: with -x -f gzip — <infile> is any number of gzip members back to back (bgzip, pigz -i, cat a.gz b.gz) and <outfile> the concatenation of their
 *     outputs (zultra_memory_decompress_members: runs of BGZF members are indexed and inflated on the device in one batch). No dictionary. With -v
 *     the members, the index's tiles and the tiles walked again are printed.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <errno.h>
#include <sys/stat.h>

#include "../../include/libzultra.h"
#include "../../include/zultra_hip.h"

static double now_s(void) {
   struct timespec ts;
   clock_gettime(CLOCK_MONOTONIC, &ts);
   return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* -f bgzf: the whole file through zultra_memory_compress_bgzf */
static int write_bgzf(FILE *fin, FILE *fout, unsigned block, int verbose, int verify, const char *gzi_name) {
   size_t n = 0, cap = (size_t)1 << 20;
   unsigned char *in = (unsigned char *)malloc(cap);
   for (size_t got; in && (got = fread(in + n, 1, cap - n, fin)) > 0;) {
      n += got;
      if (n == cap) {
         unsigned char *more = (unsigned char *)realloc(in, cap *= 2);
         if (!more) free(in);
         in = more;
      }
   }
   const size_t room = zultra_memory_bound_bgzf(n, block);
   unsigned char *out = in ? (unsigned char *)malloc(room) : NULL;
   if (!out) {
      fprintf(stderr, "out of memory\n");
      free(in);
      return 100;
   }
   const double t0 = now_s();
   const size_t size = zultra_memory_compress_bgzf(in, n, out, room, block);
   const double dt = now_s() - t0;
   int rc = 0;
   if (size == (size_t)-1) {
      fprintf(stderr, "compression error (a failed verification, a device failure, or no HIP device: this library has no CPU path)\n");
      rc = 100;
   }
   else if (fwrite(out, 1, size, fout) != size) {
      fprintf(stderr, "write error\n");
      rc = 100;
   }
   if (verbose && !rc)
      fprintf(stdout, "%llu -> %llu bytes (%.2f %%), %.1f MB/s\n", (unsigned long long)n, (unsigned long long)size, n ? 100.0 * (double)size / (double)n : 0.0, dt > 0 ? (double)n / dt / 1e6 : 0.0);
   if (verbose && verify && !rc) fprintf(stdout, "verified %llu bytes on the device\n", zultra_verified_bytes());
   if (gzi_name && !rc) {   /* -i: the index of what was written */
      const size_t gzi_size = zultra_memory_index_gzi(out, size, NULL, 0);
      unsigned char *gzi = gzi_size != (size_t)-1 ? (unsigned char *)malloc(gzi_size) : NULL;
      FILE *fgzi = gzi ? fopen(gzi_name, "wb") : NULL;
      if (!fgzi || zultra_memory_index_gzi(out, size, gzi, gzi_size) != gzi_size || fwrite(gzi, 1, gzi_size, fgzi) != gzi_size) {
         fprintf(stderr, "error writing the index '%s'\n", gzi_name);
         rc = 100;
      }
      else if (verbose)
         fprintf(stdout, "index: %llu entries\n", (unsigned long long)((gzi_size - 8) / 16));
      if (fgzi) fclose(fgzi);
      free(gzi);
   }
   zultra_release_cached_contexts();
   free(in);
   free(out);
   return rc;
}

/* -a: the files named through zultra_memory_compress_zip; with -b (block != 0) through zultra_memory_compress_zip_streams, which takes files of any size */
static int write_zip(const char *archive, char **files, int n, int verbose, int verify, unsigned block) {
   const size_t largest = block ? (size_t)0xFFFFFFFEu : 2097152;
   size_t *in_off = (size_t *)calloc((size_t)n, sizeof(size_t)), *in_size = (size_t *)calloc((size_t)n, sizeof(size_t)), *name_off = (size_t *)calloc((size_t)n + 1, sizeof(size_t));
   size_t total = 0, cap = (size_t)1 << 20, names_total = 0;
   unsigned char *in = (unsigned char *)malloc(cap), *out = NULL;
   char *names = NULL;
   int rc = in && in_off && in_size && name_off ? 0 : 100;
   for (int k = 0; k < n && !rc; k++) {
      FILE *f = fopen(files[k], "rb");
      if (!f) {
         fprintf(stderr, "error opening '%s' for reading\n", files[k]);
         rc = 100;
         break;
      }
      in_off[k] = total;
      for (size_t got = 1; got > 0 && total - in_off[k] <= largest;) {
         if (total == cap) {
            unsigned char *more = (unsigned char *)realloc(in, cap *= 2);
            if (!more) {
               rc = 100;
               break;
            }
            in = more;
         }
         total += got = fread(in + total, 1, cap - total, f);
      }
      fclose(f);
      in_size[k] = total - in_off[k];
      if (in_size[k] > largest) {
         fprintf(stderr, block ? "'%s' reaches 4 GiB: ZIP64 entries are not written\n" : "'%s' is larger than 2 MiB: an entry is one max-block (-b <max block size> takes larger files)\n", files[k]);
         rc = 100;
      }
      name_off[k] = names_total;
      names_total += strlen(files[k]);
      name_off[k + 1] = names_total;
   }
   if (!rc) {
      names = (char *)malloc(names_total + 1);
      for (int k = 0; names && k < n; k++) memcpy(names + name_off[k], files[k], name_off[k + 1] - name_off[k]);
      size_t room = zultra_memory_bound_zip(total, names_total, (size_t)n);
      if (block) {   /* (every stream at its bound, both copies of the names, the headers, the end records) */
         room = 2 * names_total + 76 * (size_t)n + 98;
         for (int k = 0; k < n; k++) room += zultra_memory_bound(in_size[k], ZULTRA_FLAG_DEFLATE_FRAMING, block);
      }
      out = (unsigned char *)malloc(room);
      FILE *fout = names && out ? fopen(archive, "wb") : NULL;
      if (!names || !out)
         fprintf(stderr, "out of memory\n");
      else if (!fout)
         fprintf(stderr, "error opening '%s' for writing\n", archive);
      rc = fout ? 0 : 100;
      if (fout) {
         const double t0 = now_s();
         const size_t size = block ? zultra_memory_compress_zip_streams(in, total, in_off, in_size, names, name_off, (size_t)n, out, room, 0, block)
                                   : zultra_memory_compress_zip(in, total, in_off, in_size, names, name_off, (size_t)n, out, room, 0);
         const double dt = now_s() - t0;
         if (size == (size_t)-1) {
            fprintf(stderr, "compression error (a failed verification, an empty or overlong name,%s a device failure, or no HIP device: this library has no CPU path)\n",
                    block ? " a file of more max-blocks than a device batch holds," : "");
            rc = 100;
         }
         else if (fwrite(out, 1, size, fout) != size) {
            fprintf(stderr, "write error\n");
            rc = 100;
         }
         if (verbose && !rc)
            fprintf(stdout, "%d entries, %llu -> %llu bytes (%.2f %%), %.1f MB/s\n", n, (unsigned long long)total, (unsigned long long)size, total ? 100.0 * (double)size / (double)total : 0.0,
                    dt > 0 ? (double)total / dt / 1e6 : 0.0);
         if (verbose && verify && !rc) fprintf(stdout, "verified %llu bytes on the device\n", zultra_verified_bytes());
         fclose(fout);
      }
   }
   else if (!in || !in_off || !in_size || !name_off)
      fprintf(stderr, "out of memory\n");
   zultra_release_cached_contexts();
   free(in);
   free(out);
   free(names);
   free(in_off);
   free(in_size);
   free(name_off);
   return rc;
}

/* mkdir -p of `path` (a directory), or of the directories in front of its last component (a file) */
static int make_dirs(char *path, int is_dir) {
   for (char *p = path + 1;; p++) {
      if (*p == '/' || (*p == 0 && is_dir)) {
         const char keep = *p;
         *p = 0;
         const int bad = mkdir(path, 0777) != 0 && errno != EEXIST;
         *p = keep;
         if (bad) return -1;
      }
      if (*p == 0) return 0;
   }
}

/* a name that stays under the directory it is unpacked into */
static int name_is_safe(const unsigned char *name, size_t n) {
   if (n == 0 || name[0] == '/') return 0;
   for (size_t i = 0, start = 0; i <= n; i++) {
      if (i < n && (name[i] == 0 || name[i] == '\\')) return 0;
      if (i == n || name[i] == '/') {
         if (i - start == 2 && name[start] == '.' && name[start + 1] == '.') return 0;
         start = i + 1;
      }
   }
   return 1;
}

/* -x -a: the archive through zultra_memory_decompress_zip, listed first, then decoded; its entries written under outdir */
static int extract_zip(const char *archive, const char *outdir, int verbose, int device) {
   FILE *fin = fopen(archive, "rb");
   if (!fin) {
      fprintf(stderr, "error opening '%s' for reading\n", archive);
      return 100;
   }
   size_t n = 0, cap = (size_t)1 << 20;
   unsigned char *in = (unsigned char *)malloc(cap), *out = NULL;
   for (size_t got; in && (got = fread(in + n, 1, cap - n, fin)) > 0;) {
      n += got;
      if (n == cap) {
         unsigned char *more = (unsigned char *)realloc(in, cap *= 2);
         if (!more) free(in);
         in = more;
      }
   }
   fclose(fin);
   zultra_zip_end_t end;
   zultra_zip_info_t *info = NULL;
   char *path = NULL;
   int rc = 100;
   const size_t tail = n < 65535 + 22 + 20 + 56 ? n : 65535 + 22 + 20 + 56;
   if (!in)
      fprintf(stderr, "out of memory\n");
   else if (zultra_zip_find_end(in + n - tail, tail, n, &end) != 0 || end.nEntries > n / 46)
      fprintf(stderr, "'%s' is no ZIP archive (no end record, or one of several disks)\n", archive);
   else {
      const size_t entries = (size_t)end.nEntries;
      size_t listed = 0, longest = 0;
      info = (zultra_zip_info_t *)calloc(entries ? entries : 1, sizeof(*info));
      const double t0 = now_s();
      const size_t total = info ? zultra_memory_decompress_zip(in, n, NULL, 0, info, entries, &listed) : (size_t)-1;
      int safe = total != (size_t)-1;
      if (!safe) fprintf(stderr, "the central directory of '%s' does not read (damaged, or no HIP device: this library has no CPU path)\n", archive);
      for (size_t i = 0; safe && i < entries; i++) {
         if (!name_is_safe(in + info[i].nNameAt, info[i].nNameLen)) {
            fprintf(stderr, "entry %llu has a name that is empty, absolute or holds '..', a backslash or a NUL byte: nothing is unpacked\n", (unsigned long long)i);
            safe = 0;
         }
         if (info[i].nNameLen > longest) longest = info[i].nNameLen;
      }
      out = safe ? (unsigned char *)malloc(total ? total : 1) : NULL;
      path = safe ? (char *)malloc(strlen(outdir) + longest + 2) : NULL;
      if (safe && (!out || !path)) fprintf(stderr, "out of memory\n");
      if (out && path) {
         const size_t size = zultra_memory_decompress_zip(in, n, out, total, info, entries, &listed);
         const double dt = now_s() - t0;
         if (size == (size_t)-1) {
            fprintf(stderr, "decompression error:");
            for (size_t i = 0; i < entries; i++)
               if (info[i].nStatus) fprintf(stderr, " entry %llu '%.*s' reason %u;", (unsigned long long)i, (int)info[i].nNameLen, (const char *)in + info[i].nNameAt, info[i].nStatus);
            fprintf(stderr, " (reasons: include/zultra_hip.h, zultra_hip_unzip) nothing is unpacked\n");
         }
         else {
            rc = 0;
            for (size_t i = 0; i < entries && !rc; i++) {
               const int is_dir = in[info[i].nNameAt + info[i].nNameLen - 1] == '/';
               sprintf(path, "%s/%.*s", outdir, (int)info[i].nNameLen, (const char *)in + info[i].nNameAt);
               FILE *f = make_dirs(path, is_dir) == 0 && !is_dir ? fopen(path, "wb") : NULL;
               if (!is_dir && (!f || fwrite(out + info[i].nOutOff, 1, info[i].nSize, f) != info[i].nSize)) {
                  fprintf(stderr, "error writing '%s'\n", path);
                  rc = 100;
               }
               if (f) fclose(f);
               if (verbose && !rc)
                  fprintf(stdout, "%10u -> %10u  %s  %08x  %.*s\n", info[i].nCompSize, info[i].nSize, info[i].nMethod == 8 ? "deflated" : "stored  ", info[i].nCrc32, (int)info[i].nNameLen,
                          (const char *)in + info[i].nNameAt);
            }
            if (!entries && make_dirs(strcpy(path, outdir), 1) != 0) rc = 100;
         }
         if (verbose && !rc) {
            zultra_hip_zip_index_result_t ix;
            memset(&ix, 0, sizeof(ix));
            /* zultra_memory_decompress_zip does not hand its index result on, so the counts come from an index of the directory's bytes alone, as a source
             * of their own: the tiles are cut from the directory's start, so they are the same ones, and only the directory is uploaded again */
            if (end.nCentralSize) (void)zultra_hip_zip_index(device, in + end.nPrefix + end.nCentralOff, (size_t)end.nCentralSize, 0, 0, end.nCentralSize, NULL, 0, &ix, NULL);
            fprintf(stdout, "%llu entries, %llu -> %llu bytes, %.1f MB/s; the directory index: %u tiles, %u rewalked\n", (unsigned long long)entries, (unsigned long long)n, (unsigned long long)size,
                    dt > 0 ? (double)size / dt / 1e6 : 0.0, ix.tiles, ix.tiles_rewalked);
         }
      }
   }
   free(in);
   free(out);
   free(info);
   free(path);
   return rc;
}

/* -x: the whole file through zultra_memory_decompress. The output size is not known in advance (gzip's ISIZE is a hint, modulo 2^32): the buffer
 * grows until the call succeeds or the bound of the format is passed (a deflate stream expands at most 1032 : 1). */
static int extract(FILE *fin, FILE *fout, unsigned flags, int verbose, const void *dict, int dict_size, int members, int device) {
   size_t n = 0, cap = (size_t)1 << 20;
   unsigned char *in = (unsigned char *)malloc(cap);
   for (size_t got; in && (got = fread(in + n, 1, cap - n, fin)) > 0;) {
      n += got;
      if (n == cap) in = (unsigned char *)realloc(in, cap *= 2);
   }
   if (!in) {
      fprintf(stderr, "out of memory\n");
      return 100;
   }
   const size_t bound = n * 1032 + 1024;
   size_t room = n * 4 + 4096, size = (size_t)-1;
   if ((flags & ZULTRA_FLAG_GZIP_FRAMING) && n >= 18) room = (size_t)in[n - 4] | ((size_t)in[n - 3] << 8) | ((size_t)in[n - 2] << 16) | ((size_t)in[n - 1] << 24);
   /* -m: where the whole file indexes (a BGZF file), the index says how much room it needs; else the buffer grows as above */
   zultra_hip_index_result_t ix;
   memset(&ix, 0, sizeof(ix));
   size_t nmembers = 0;
   const int indexed = members && n && zultra_hip_index_members(device, in, n, 0, NULL, 0, &ix, NULL) == 0;
   if (indexed && ix.stop == 0) room = (size_t)ix.out_size;
   else if (members) room = n * 4 + 4096;   /* (the last member's ISIZE says nothing about the others) */
   const double t0 = now_s();
   unsigned char *out = NULL;
   for (;;) {
      if (room > bound) room = bound;
      free(out);
      out = (unsigned char *)malloc(room ? room : 1);
      if (!out) break;
      size = members ? zultra_memory_decompress_members(in, n, out, room, &nmembers)
             : dict  ? zultra_memory_decompress_dict(in, n, out, room, flags, dict, dict_size)
                     : zultra_memory_decompress(in, n, out, room, flags);
      if (size != (size_t)-1 || room == bound) break;
      room = room < 4096 ? 8192 : room * 2;
   }
   const double dt = now_s() - t0;
   int rc = 0;
   if (size == (size_t)-1) {
      fprintf(stderr, "decompression error (a damaged stream, another framing than -f names, another dictionary than -D names or none, or no HIP device: this library has no CPU path)\n");
      rc = 100;
   }
   else if (size && fwrite(out, 1, size, fout) != size) {
      fprintf(stderr, "write error\n");
      rc = 100;
   }
   if (verbose && !rc) fprintf(stdout, "%llu -> %llu bytes, %.1f MB/s\n", (unsigned long long)n, (unsigned long long)size, dt > 0 ? (double)size / dt / 1e6 : 0.0);
   if (verbose && !rc && members)
      fprintf(stdout, "%llu members; the index from the start of the file: %u members, %u tiles, %u rewalked\n", (unsigned long long)nmembers, ix.members, ix.tiles, ix.tiles_rewalked);
   free(in);
   free(out);
   return rc;
}

/* a whole file in memory; NULL (and a message) where it does not read */
static unsigned char *read_file(FILE *f, size_t *size) {
   size_t n = 0, cap = (size_t)1 << 20;
   unsigned char *in = (unsigned char *)malloc(cap);
   for (size_t got; in && (got = fread(in + n, 1, cap - n, f)) > 0;) {
      n += got;
      if (n == cap) {
         unsigned char *more = (unsigned char *)realloc(in, cap *= 2);
         if (!more) free(in);
         in = more;
      }
   }
   if (!in) fprintf(stderr, "out of memory\n");
   *size = n;
   return in;
}

/* -x -m -r: bytes first .. first + length of the file's output through zultra_memory_decompress_range, with the .gzi index where one is named */
static int extract_range(FILE *fin, FILE *fout, unsigned long long first, unsigned long long length, const char *gzi_name, int verbose, int device) {
   size_t n = 0, gzi_size = 0;
   unsigned char *in = read_file(fin, &n), *gzi = NULL, *out = NULL;
   int rc = in ? 0 : 100;
   if (!rc && gzi_name) {
      FILE *fgzi = fopen(gzi_name, "rb");
      gzi = fgzi ? read_file(fgzi, &gzi_size) : NULL;
      if (fgzi) fclose(fgzi);
      if (!gzi) {
         fprintf(stderr, "error reading the index '%s'\n", gzi_name);
         rc = 100;
      }
   }
   const unsigned long long bound = (unsigned long long)n * 1032 + 1024;   /* (a deflate stream expands at most 1032 : 1) */
   const size_t room = (size_t)(length < bound ? length : bound);
   if (!rc && !(out = (unsigned char *)malloc(room ? room : 1))) {
      fprintf(stderr, "out of memory\n");
      rc = 100;
   }
   if (!rc) {
      const double t0 = now_s();
      const size_t size = zultra_memory_decompress_range(in, n, first, room, out, room, gzi, gzi_size);
      const double dt = now_s() - t0;
      if (size == (size_t)-1) {
         fprintf(stderr, "decompression error (a damaged member in the range, no BGZF file, an index that does not fit the file, or no HIP device: this library has no CPU path)\n");
         rc = 100;
      }
      else if (size && fwrite(out, 1, size, fout) != size) {
         fprintf(stderr, "write error\n");
         rc = 100;
      }
      if (verbose && !rc) {
         zultra_hip_range_result_t rg;
         memset(&rg, 0, sizeof(rg));
         (void)zultra_hip_inflate_range(device, in, n, 0, first, room, out, 0, 0, &rg, NULL, 0, NULL);   /* (no room: a query, nothing is decoded) */
         fprintf(stdout, "%llu bytes from %llu, %.1f MB/s; first member %u, %u members of %u; the index: %u tiles, %u rewalked\n", (unsigned long long)size, first,
                 dt > 0 ? (double)size / dt / 1e6 : 0.0, rg.first_member, rg.range_members, rg.members, rg.tiles, rg.tiles_rewalked);
      }
   }
   free(in);
   free(gzi);
   free(out);
   return rc;
}

int main(int argc, char **argv) {
   unsigned flags = ZULTRA_FLAG_GZIP_FRAMING, block = 0;
   size_t chunk = (size_t)8 << 20;
   int verbose = 0, verify = 0, do_extract = 0, members = 0, device = 0, bgzf = 0, i = 1;
   const char *dict_name = NULL, *archive = NULL, *range = NULL, *gzi_name = NULL;
   unsigned long long range_first = 0, range_length = 0;
   if (getenv("ZULTRA_HIP_DEVICE")) device = atoi(getenv("ZULTRA_HIP_DEVICE"));   /* (the library's own default: -m sizes its buffer with an index call on the same device) */
   for (; i < argc && argv[i][0] == '-' && argv[i][1]; i++) {
      if (!strcmp(argv[i], "-b") && i + 1 < argc)
         block = (unsigned)strtoul(argv[++i], NULL, 0);
      else if (!strcmp(argv[i], "-k") && i + 1 < argc)
         chunk = (size_t)strtoul(argv[++i], NULL, 0) << 10;
      else if (!strcmp(argv[i], "-d") && i + 1 < argc)
         zultra_set_device(device = atoi(argv[++i]));
      else if (!strcmp(argv[i], "-f") && i + 1 < argc) {
         const char *f = argv[++i];
         bgzf = !strcmp(f, "bgzf");
         flags = !strcmp(f, "gzip") || bgzf ? ZULTRA_FLAG_GZIP_FRAMING : !strcmp(f, "zlib") ? ZULTRA_FLAG_ZLIB_FRAMING : ZULTRA_FLAG_DEFLATE_FRAMING;
      }
      else if (!strcmp(argv[i], "-D") && i + 1 < argc)
         dict_name = argv[++i];
      else if (!strcmp(argv[i], "-a") && i + 1 < argc)
         archive = argv[++i];
      else if (!strcmp(argv[i], "-r") && i + 1 < argc)
         range = argv[++i];
      else if (!strcmp(argv[i], "-i") && i + 1 < argc)
         gzi_name = argv[++i];
      else if (!strcmp(argv[i], "-v"))
         verbose = 1;
      else if (!strcmp(argv[i], "-x"))
         do_extract = 1;
      else if (!strcmp(argv[i], "-m"))
         members = 1;
      else if (!strcmp(argv[i], "-c")) {
         verify = 1;
         zultra_set_verify(1);
      }
      else
         break;
   }
   if (bgzf && !do_extract && block > ZULTRA_HIP_BGZF_BLOCK) {
      fprintf(stderr, "-b %u: a BGZF block holds at most %u bytes of input\n", block, ZULTRA_HIP_BGZF_BLOCK);
      return 100;
   }
   int range_ok = 1;
   if (range) {   /* <first>:<length>, both decimal */
      char *end = NULL;
      range_first = strtoull(range, &end, 10);
      range_ok = end != range && *end == ':' && end[1] >= '0' && end[1] <= '9';
      if (range_ok) {
         const char *len = end + 1;
         range_length = strtoull(len, &end, 10);
         range_ok = *end == 0;
      }
   }
   if (!range_ok || (range && (!members || archive)) || (gzi_name && !(range || (bgzf && !do_extract)))) {
      fprintf(stderr, "-r <first>:<length> goes with -x -m; -i <file.gzi> with -f bgzf (written) or with -x -m -r (read)\n");
      return 100;
   }
   if (archive ? ((do_extract ? argc - i != 1 || members || verify : argc - i < 1) || bgzf || dict_name) : argc - i != 2 || chunk == 0 || (members && (!do_extract || flags != ZULTRA_FLAG_GZIP_FRAMING || dict_name)) || (bgzf && !do_extract && dict_name)) {
      fprintf(stderr, "usage: %s [-b <max block size>] [-f gzip|zlib|raw] [-k <chunk KiB>] [-d <device>] [-D <dictionary>] [-c] [-v] <infile> <outfile>\n"
                      "       %s -x [-f gzip|zlib|raw] [-d <device>] [-D <dictionary>] [-v] <infile> <outfile>\n"
                      "       %s -x -m [-f gzip] [-d <device>] [-v] <infile> <outfile>   (any number of gzip members: BGZF, pigz -i, cat a.gz b.gz)\n"
                      "       %s -x -m -r <first>:<length> [-i <file.gzi>] [-f gzip] [-d <device>] [-v] <infile> <outfile>   (a byte range of a BGZF file's output)\n"
                      "       %s -f bgzf [-b <block size, at most 65280>] [-i <file.gzi>] [-d <device>] [-c] [-v] <infile> <outfile>   (BGZF members and the end marker)\n"
                      "       %s -a <archive.zip> [-b <max block size>] [-d <device>] [-c] [-v] <file>...   (a ZIP archive: every file an entry under its name; of at most 2 MiB without -b)\n"
                      "       %s -x -a <archive.zip> [-d <device>] [-v] <outdir>   (unpack a ZIP archive: stored and deflated entries, checked on the device)\n", argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0]);
      return 100;
   }
   if (archive && do_extract) return extract_zip(archive, argv[i], verbose, device);
   if (archive) return write_zip(archive, argv + i, argc - i, verbose, verify, block);
   void *dict = NULL;
   int dict_size = 0;
   if (dict_name && (zultra_dictionary_load(dict_name, &dict, &dict_size) != ZULTRA_OK || dict_size <= 0)) {
      fprintf(stderr, "error loading dictionary '%s'\n", dict_name);
      zultra_dictionary_free(&dict);
      return 100;
   }
   FILE *fin = fopen(argv[i], "rb");
   if (!fin) {
      fprintf(stderr, "error opening '%s' for reading\n", argv[i]);
      return 100;
   }
   FILE *fout = fopen(argv[i + 1], "wb");
   if (!fout) {
      fprintf(stderr, "error opening '%s' for writing\n", argv[i + 1]);
      fclose(fin);
      return 100;
   }
   if (do_extract && range) {
      const int xrc = extract_range(fin, fout, range_first, range_length, gzi_name, verbose, device);
      fclose(fin);
      fclose(fout);
      return xrc;
   }
   if (do_extract) {
      const int xrc = extract(fin, fout, flags, verbose, dict, dict_size, members, device);
      fclose(fin);
      fclose(fout);
      zultra_dictionary_free(&dict);
      return xrc;
   }
   if (bgzf) {
      const int brc = write_bgzf(fin, fout, block, verbose, verify, gzi_name);
      fclose(fin);
      fclose(fout);
      return brc;
   }
   unsigned char *in = (unsigned char *)malloc(chunk), *out = (unsigned char *)malloc(chunk);
   zultra_stream_t strm;
   memset(&strm, 0, sizeof(strm));
   if (!in || !out || zultra_stream_init(&strm, flags, block) != ZULTRA_OK) {
      fprintf(stderr, "error initializing compressor (no HIP device? this library has no CPU path)\n");
      return 100;
   }
   if (dict && zultra_stream_set_dictionary(&strm, dict, dict_size) != ZULTRA_OK) {
      fprintf(stderr, "error setting the dictionary\n");
      return 100;
   }
   const double t0 = now_s();
   int status = ZULTRA_OK, eof = 0, rc = 0;
   while (status == ZULTRA_OK) {
      if (!strm.avail_in && !eof) {
         strm.next_in = in;
         strm.avail_in = fread(in, 1, chunk, fin);
         eof = strm.avail_in < chunk;   /* as the reference's tool: a short read ends the input (tool/zultra.c:161-166) */
      }
      strm.next_out = out;
      strm.avail_out = chunk;
      status = zultra_stream_compress(&strm, eof ? ZULTRA_FINALIZE : ZULTRA_CONTINUE);
      const size_t produced = chunk - strm.avail_out;
      if (produced && fwrite(out, 1, produced, fout) != produced) {
         fprintf(stderr, "write error\n");
         rc = 100;
         break;
      }
   }
   if (status != ZULTRA_STREAM_END && !rc) {
      fprintf(stderr, "compression error %d\n", status);
      rc = 100;
   }
   const double dt = now_s() - t0;
   if (verbose && !rc)
      fprintf(stdout, "%llu -> %llu bytes (%.2f %%), %.1f MB/s\n", (unsigned long long)strm.total_in, (unsigned long long)strm.total_out,
              strm.total_in ? 100.0 * (double)strm.total_out / (double)strm.total_in : 0.0, dt > 0 ? (double)strm.total_in / dt / 1e6 : 0.0);
   if (verbose && verify && !rc) fprintf(stdout, "verified %llu bytes on the device\n", zultra_verified_bytes());
   zultra_stream_end(&strm);
   zultra_release_cached_contexts();
   zultra_dictionary_free(&dict);
   free(in);
   free(out);
   fclose(fin);
   fclose(fout);
   return rc;
}
