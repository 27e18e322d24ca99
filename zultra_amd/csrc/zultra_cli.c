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
 *    zultra_amd_cli -f bgzf [-b <block size>] [-d <device>] [-c] [-v] <infile> <outfile>
 *    zultra_amd_cli -a <archive.zip> [-d <device>] [-c] [-v] <file>...
 *
 * -a: a ZIP archive of the files named, every file an entry under its name as given, headers and central directory written on the device
 *     (zultra_memory_compress_zip). A file is one max-block: at most 2 MiB; an empty file is an empty entry. No dictionary.
 * -f bgzf: bgzip(1) — <infile> in blocks of -b bytes (default and at most 65280), every block a BGZF member written on the device, and BGZF's end marker
 *     (zultra_memory_compress_bgzf); `-x -m -f gzip` is the way back. No dictionary: a member stands alone.
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

#include "../../include/libzultra.h"
#include "../../include/zultra_hip.h"

static double now_s(void) {
   struct timespec ts;
   clock_gettime(CLOCK_MONOTONIC, &ts);
   return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* -f bgzf: the whole file through zultra_memory_compress_bgzf */
static int write_bgzf(FILE *fin, FILE *fout, unsigned block, int verbose, int verify) {
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
   zultra_release_cached_contexts();
   free(in);
   free(out);
   return rc;
}

/* -a: the files named through zultra_memory_compress_zip */
static int write_zip(const char *archive, char **files, int n, int verbose, int verify) {
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
      for (size_t got = 1; got > 0 && total - in_off[k] <= 2097152;) {
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
      if (in_size[k] > 2097152) {
         fprintf(stderr, "'%s' is larger than 2 MiB: an entry is one max-block\n", files[k]);
         rc = 100;
      }
      name_off[k] = names_total;
      names_total += strlen(files[k]);
      name_off[k + 1] = names_total;
   }
   if (!rc) {
      names = (char *)malloc(names_total + 1);
      for (int k = 0; names && k < n; k++) memcpy(names + name_off[k], files[k], name_off[k + 1] - name_off[k]);
      const size_t room = zultra_memory_bound_zip(total, names_total, (size_t)n);
      out = (unsigned char *)malloc(room);
      FILE *fout = names && out ? fopen(archive, "wb") : NULL;
      if (!names || !out)
         fprintf(stderr, "out of memory\n");
      else if (!fout)
         fprintf(stderr, "error opening '%s' for writing\n", archive);
      rc = fout ? 0 : 100;
      if (fout) {
         const double t0 = now_s();
         const size_t size = zultra_memory_compress_zip(in, total, in_off, in_size, names, name_off, (size_t)n, out, room, 0);
         const double dt = now_s() - t0;
         if (size == (size_t)-1) {
            fprintf(stderr, "compression error (a failed verification, an empty or overlong name, a device failure, or no HIP device: this library has no CPU path)\n");
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

int main(int argc, char **argv) {
   unsigned flags = ZULTRA_FLAG_GZIP_FRAMING, block = 0;
   size_t chunk = (size_t)8 << 20;
   int verbose = 0, verify = 0, do_extract = 0, members = 0, device = 0, bgzf = 0, i = 1;
   const char *dict_name = NULL, *archive = NULL;
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
   if (archive ? (argc - i < 1 || do_extract || bgzf || dict_name) : argc - i != 2 || chunk == 0 || (members && (!do_extract || flags != ZULTRA_FLAG_GZIP_FRAMING || dict_name)) || (bgzf && !do_extract && dict_name)) {
      fprintf(stderr, "usage: %s [-b <max block size>] [-f gzip|zlib|raw] [-k <chunk KiB>] [-d <device>] [-D <dictionary>] [-c] [-v] <infile> <outfile>\n"
                      "       %s -x [-f gzip|zlib|raw] [-d <device>] [-D <dictionary>] [-v] <infile> <outfile>\n"
                      "       %s -x -m [-f gzip] [-d <device>] [-v] <infile> <outfile>   (any number of gzip members: BGZF, pigz -i, cat a.gz b.gz)\n"
                      "       %s -f bgzf [-b <block size, at most 65280>] [-d <device>] [-c] [-v] <infile> <outfile>   (BGZF members and the end marker)\n"
                      "       %s -a <archive.zip> [-d <device>] [-c] [-v] <file>...   (a ZIP archive: every file, of at most 2 MiB, an entry under its name)\n", argv[0], argv[0], argv[0], argv[0], argv[0]);
      return 100;
   }
   if (archive) return write_zip(archive, argv + i, argc - i, verbose, verify);
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
   if (do_extract) {
      const int xrc = extract(fin, fout, flags, verbose, dict, dict_size, members, device);
      fclose(fin);
      fclose(fout);
      zultra_dictionary_free(&dict);
      return xrc;
   }
   if (bgzf) {
      const int brc = write_bgzf(fin, fout, block, verbose, verify);
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
