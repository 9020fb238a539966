/*
 * mdc_zipw.h -- C interface of libmdc_zipw.so: ZIP archives of stored files, built on the device from device-resident bytes.
 *
 * The input of every device function is what mdcj_encode_*_device (include/mdc_jenc.h) leaves: file f at d_data + f * slot_bytes
 * (a 64-bit offset), its length in int32_t d_sizes[f].  Nothing here knows about JPEG: any batch of device-resident byte strings
 * is archived.  A library of its own: it links none of libmdc_hip.so / libmdc_host.so / libmdc_jenc.so, none of them links it,
 * and it needs no mdc_ctx.
 *
 * CRC-32 is zlib's crc32(): reflected polynomial 0xEDB88320, initial value and final XOR 0xFFFFFFFF; a file of 0 bytes gives 0.
 *
 * The archive is a pure function of its files.  Every local file header is
 *   "PK\3\4", version needed 20, flags 0, method 0 (stored), DOS time 0, DOS date 0x0021 (1980-01-01), the CRC-32, compressed
 *   size = uncompressed size = the file's size, name length, extra length 0, then the name, then the file's bytes.
 * An entry's name is its index (first_index + f) printed as %05d -- longer past 99999, as %05d does -- followed by a suffix of
 * at most MDCZ_MAX_SUFFIX ASCII bytes (".jpg").  The central directory (mdcz_directory) repeats these fields with version made by
 * 20 / Unix (0x0314), attributes 0, and adds the ZIP64 pieces only where the format needs them (see there).
 *
 * Limits, each checked and reported as an error status (never a fault): 0 <= nfiles <= 2^40 (64-bit); 0 <= d_sizes[f] <= 2^31 - 1 (a
 * negative size on the device is taken as 0 by the kernels and refused by the writer, which reads the sizes); any slot_bytes >= 0
 * and any alignment of d_data; 0 <= first_index and first_index + nfiles <= 10^18; suffix: at most 15 bytes, each below 0x80.
 * The scratch arrays of a call (4 bytes per file and part, see mdcz_crc_geometry) are taken from and returned to the stream's
 * memory pool (hipMallocAsync / hipFreeAsync): MDCZ_ERR_NOMEM when that fails.
 *
 * Threads: the device functions enqueue on `stream` (hipStream_t as void*, NULL = the default stream) and do not synchronise.
 * Calls on one writer are ordered by the caller; different writers are independent, also on one stream.
 */
#ifndef MDC_ZIPW_H
#define MDC_ZIPW_H
#include <stddef.h>
#include <stdint.h>
#ifndef MDC_API
#if defined(__GNUC__) || defined(__clang__)
#define MDC_API __attribute__((visibility("default")))
#else
#define MDC_API
#endif
#endif
#ifdef __cplusplus
extern "C" {
#endif

#define MDCZ_OK 0
#define MDCZ_ERR_ARG (-1)       /* null pointer, negative count or size, bad suffix or index */
#define MDCZ_ERR_STATE (-2)     /* the sizes on the device changed during an append */
#define MDCZ_ERR_SIZE (-3)      /* a capacity below the bound */
#define MDCZ_ERR_HIP (-4)       /* a HIP call failed */
#define MDCZ_ERR_NO_DEVICE (-5) /* no such HIP device */
#define MDCZ_ERR_NOMEM (-6)     /* scratch or staging memory could not be allocated */
#define MDCZ_ERR_IO (-7)        /* open / write / close failed: the message carries errno's text */

#define MDCZ_MAX_SUFFIX 15
#define MDCZ_NAME_STRIDE 40 /* bytes per name in mdcz_directory's `names` array: up to 19 digits + 15 suffix bytes + NUL */

/* One per input file, written by mdcz_segment_device: where the file's local header starts inside the segment (-1: the file was
 * left out), its CRC-32 and its size.  Record nfiles, one past the last file, holds the segment's length in `offset`. */
typedef struct mdcz_record {
  int64_t offset;
  uint32_t crc;
  uint32_t size;
} mdcz_record;

typedef struct mdcz_writer mdcz_writer;

/* The message of the calling thread's last failed mdcz_* call ("" if none). */
MDC_API const char* mdcz_last_error(void);

/* How the checksum kernel cuts a file, for tests and tools: out[0] = bytes per load (16), out[1] = distance between the
 * consecutive words of one lane (one workgroup row), out[2] = bytes one wave covers per row, out[3] = bytes one workgroup covers per
 * row, out[4] = the number of parts (workgroups) a file is split over for a call with this slot_bytes and nfiles: part p takes
 * rows [p * R, (p + 1) * R) of the file's 16-byte-aligned body, R = ceil(rows / parts). */
MDC_API void mdcz_crc_geometry(int64_t slot_bytes, int64_t nfiles, int64_t* out);

/* d_crc[f] = CRC-32 of the d_sizes[f] bytes at d_data + f * slot_bytes, f = 0 .. nfiles - 1. */
MDC_API int mdcz_crc32_device(const uint8_t* d_data, int64_t slot_bytes, const int32_t* d_sizes, int64_t nfiles, uint32_t* d_crc, void* stream);
/* The same with the lane's fold step chosen: 0 = four 256-entry table lookups from LDS (what mdcz_crc32_device uses), 1 = 32
 * shift-and-XOR steps.  For tools/zipw_rate.py. */
MDC_API int mdcz_crc32_variant_device(int variant, const uint8_t* d_data, int64_t slot_bytes, const int32_t* d_sizes, int64_t nfiles, uint32_t* d_crc,
                                      void* stream);

/* Upper bound in bytes of the segment of nfiles files of total_bytes bytes in all whose names are at most max_name_len long:
 * nfiles * (30 + max_name_len) + total_bytes; -1 when an argument is negative or the sum passes 2^63 - 1. */
MDC_API int64_t mdcz_segment_bound(int64_t nfiles, int64_t total_bytes, int max_name_len);

/* For every file whose d_valid[f] is non-zero (d_valid NULL: every file), in index order and back to back into d_segment: local
 * header, name, bytes.  d_records gets nfiles + 1 records (above).  CRC, offsets (a device scan over 30 + name length + size) and
 * the gather run on `stream` with no host round trip between them.  When the segment's length passes segment_capacity nothing is
 * written to d_segment (the records are, so record nfiles tells the caller); nothing at or past the length is ever written. */
MDC_API int mdcz_segment_device(const uint8_t* d_data, int64_t slot_bytes, const int32_t* d_sizes, const uint8_t* d_valid, int64_t nfiles,
                                int64_t first_index, const char* suffix, uint8_t* d_segment, int64_t segment_capacity, mdcz_record* d_records,
                                void* stream);

/* Pure host function, no HIP call: the central directory and the end records of an archive whose entries are records[i] with
 * offset >= 0 (others are skipped), entry i's local header at segment_base_offset + records[i].offset and its name the
 * NUL-terminated string at names + i * MDCZ_NAME_STRIDE; the directory itself starts at directory_offset.  An entry whose
 * header offset is >= 0xFFFFFFFF carries the ZIP64 extra field (id 0x0001, 8 bytes: the offset) and version needed 45.  The
 * ZIP64 end-of-central-directory record and its locator are written when there are more than 65,534 entries or the directory's
 * offset or size is >= 0xFFFFFFFF, and not otherwise.  Returns the number of bytes (with out == NULL: the number needed, nothing
 * written), or a negative status: MDCZ_ERR_SIZE when capacity is below that number. */
MDC_API int64_t mdcz_directory(const mdcz_record* records, int64_t n, const char* names, int64_t segment_base_offset, int64_t directory_offset,
                               uint8_t* out, int64_t capacity);

/* A writer of one archive at `path` (created or truncated), fed from HIP device `device` (-1 = the calling thread's current
 * device at the first append).  No HIP call is made here.  staging_cap: a batch whose segment (plus its records) would pass this
 * many bytes is split by the writer into several segments, so the page-locked buffer and its device twin stay below it -- except
 * for a single file larger than the cap, which goes alone; <= 0 = 256 MiB. */
MDC_API int mdcz_open(const char* path, int device, int64_t staging_cap, mdcz_writer** out);
/* Appends files 0 .. nfiles - 1 (h_valid: host array, NULL = all) as entries first_index .. : CRC, scan and gather on `stream`, one
 * copy of the segment into the writer's page-locked buffer, one write() at the end of the file.  Waits for the stream. */
MDC_API int mdcz_append_device(mdcz_writer* w, const uint8_t* d_data, int64_t slot_bytes, const int32_t* d_sizes, const uint8_t* h_valid,
                               int64_t nfiles, int64_t first_index, const char* suffix, void* stream);
/* Appends the central directory, closes the file and frees the writer (also when it fails).  Returns the archive's size. */
MDC_API int64_t mdcz_close(mdcz_writer* w);
/* Closes and removes the unfinished file, frees the writer. */
MDC_API void mdcz_abort(mdcz_writer* w);

#ifdef __cplusplus
}
#endif
#endif /* MDC_ZIPW_H */
