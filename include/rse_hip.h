/*
 * rse_hip.h -- C ABI of the MI355X-native Reed-Solomon erasure-coding library
 * (librse_hip.so).  Drop-in for the hot path of rust-rse/reed-solomon-erasure
 * v6.0.0: the codec API of core.rs (ReedSolomon<F>::new / encode / encode_sep /
 * encode_single / encode_single_sep / verify / verify_with_buffer / reconstruct /
 * reconstruct_data) over the galois_8 and galois_16 fields, plus the fused
 * shard x matrix kernel that replaces code_some_slices (core.rs:481-509) and the
 * native FFI kernel reedsolomon_gal_mul(_xor) (simd_c/reedsolomon.h:30-42).
 *
 * Conventions (mirroring the reference; see INTEGRATION.md for the Rust binding):
 *  - Shards are DEVICE pointers (HBM) unless the function name ends in _host;
 *    the Field/FFI slice hooks (rse_gal_mul*, rse_gf8/gf16_mul_slice) take
 *    host or device memory.
 *  - Lengths are in field ELEMENTS, like Rust slice lengths: bytes for GF(2^8),
 *    2-byte [u8;2] elements ({coefficient of x, constant}, galois_16.rs:49-51)
 *    for GF(2^16).
 *  - Return value: RSE_OK (0), one of the 13 reference errors (errors.rs:4-18,
 *    numbered as wasm/src/lib.rs:11-24), or an RSE_ERR_* library status >= 100.
 *  - On any error nothing is written (core.rs:673-676).
 *  - Work is enqueued on `stream` (a hipStream_t; NULL = the legacy default
 *    stream) and runs asynchronously, except verify*, whose boolean result
 *    requires waiting before returning: for the stream's work up to and
 *    including the check, or (RSE_OPT_SPIN_WAIT, one compiled check-kernel
 *    launch) for the check kernel's completion word, stored after every one of
 *    its memory accesses has completed.  Either way the shards may be reused
 *    once the call returns.  Each call runs on
 *    the device that owns `stream` (NULL: the current device); the caller's
 *    current device is restored on return.
 *  - A codec is immutable after rse_codec_new except for its mutex-guarded
 *    decode-matrix LRU cache (capacity 254, core.rs:24), so concurrent calls on
 *    different streams are allowed (core.rs:349).
 *  - The caller owns all shard memory; the library never frees caller buffers.
 */
#ifndef RSE_HIP_H
#define RSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------- */
#define RSE_OK 0
/* errors.rs:4-18, in declaration order */
#define RSE_TOO_FEW_SHARDS 1
#define RSE_TOO_MANY_SHARDS 2
#define RSE_TOO_FEW_DATA_SHARDS 3
#define RSE_TOO_MANY_DATA_SHARDS 4
#define RSE_TOO_FEW_PARITY_SHARDS 5
#define RSE_TOO_MANY_PARITY_SHARDS 6
#define RSE_TOO_FEW_BUFFER_SHARDS 7
#define RSE_TOO_MANY_BUFFER_SHARDS 8
#define RSE_INCORRECT_SHARD_SIZE 9
#define RSE_TOO_FEW_SHARDS_PRESENT 10
#define RSE_EMPTY_SHARD 11
#define RSE_INVALID_SHARD_FLAGS 12
#define RSE_INVALID_INDEX 13
/* library statuses (no reference counterpart: the reference panics or cannot fail) */
#define RSE_ERR_INVALID_ARGUMENT 100 /* NULL pointer, unknown field, bad size */
#define RSE_ERR_DEVICE 101           /* HIP runtime error; see rse_last_device_error */
#define RSE_ERR_NO_MEMORY 102
#define RSE_ERR_SINGULAR_MATRIX 103  /* matrix.rs:11-13 Error::SingularMatrix */

#define RSE_FIELD_GF8 8   /* galois_8::Field,  ORDER 256   */
#define RSE_FIELD_GF16 16 /* galois_16::Field, ORDER 65536 */

typedef struct rse_codec rse_codec;
typedef void *rse_stream_t; /* hipStream_t */

/* Human-readable message; reference errors use errors.rs:20-38 verbatim. */
const char *rse_strerror(int status);
/* hipError_t of the last RSE_ERR_DEVICE on this thread (0 if none). */
int rse_last_device_error(void);
/* Library version string. */
const char *rse_version(void);
/* Identity of the last coding kernel this thread launched, e.g. "bitslice gf8
 * 10+4 v5 nt1" (compiled-in bit-sliced), "bitslice-jit gf16 12+8" (specialised
 * at run time), "table gf8 50+20 fused nt1"; "" before the first launch.
 * Diagnostics: profiles are attributed to the kernel that actually ran. */
const char *rse_last_kernel(void);

/* ---- codec: core.rs:343-923 ------------------------------------------ */
/* ReedSolomon::new (core.rs:445-467): TooFewDataShards / TooFewParityShards /
 * TooManyShards (data + parity > ORDER).  Builds the systematic matrix
 * V * (V[0..k])^-1 (core.rs:430-436) on the host; touches no device. */
int rse_codec_new(int field, size_t data_shards, size_t parity_shards, rse_codec **out);
void rse_codec_free(rse_codec *codec);
int rse_codec_field(const rse_codec *codec);
size_t rse_codec_data_shard_count(const rse_codec *codec);   /* core.rs:469 */
size_t rse_codec_parity_shard_count(const rse_codec *codec); /* core.rs:473 */
size_t rse_codec_total_shard_count(const rse_codec *codec);  /* core.rs:477 */
/* Copy the (k+p) x k encoding matrix, row-major, elem bytes per element. */
int rse_codec_matrix(const rse_codec *codec, uint8_t *out, size_t out_bytes);
/* Which kernels code this codec's whole 16 KiB and 4 KiB chunks (no reference counterpart;
 * results are identical either way).  Codecs other than the compiled-in ones get
 * bit-sliced kernels specialised at run time: the first call that codes at least
 * 4 KiB per shard (or this call with wait != 0) starts a hiprtc compile of the
 * codec's parity rows on a background thread (host CPU only) -- one module for
 * p <= 8 and k <= 32, one per 8 x 32 block of the rows otherwise.  wait != 0
 * blocks until every build has finished. */
#define RSE_KERNELS_TABLE 0             /* table kernels (rse_kernels.hip) */
#define RSE_KERNELS_COMPILED 1          /* bit-sliced, compiled into the library */
#define RSE_KERNELS_SPECIALISED 2       /* bit-sliced, specialised at run time, ready */
#define RSE_KERNELS_SPECIALISING 3      /* compile in flight (wait == 0) */
#define RSE_KERNELS_SPECIALISE_FAILED 4 /* compile failed: table kernels */
#define RSE_KERNELS_FFT 5               /* additive-FFT kernels, compiled into the library
                                           (GF(2^8) k = p = 16, 32, 64, and 128 at
                                           RSE_OPT_FFT 2; at RSE_OPT_FFT16 1, GF(2^16)
                                           codecs past 256 shards with 2^m - k <= 32) */
int rse_codec_kernel_kind(const rse_codec *codec, int wait);

/* encode (core.rs:597-611): shards[0..k] data, shards[k..k+p] parity (overwritten). */
int rse_encode(const rse_codec *codec, void *const *shards, const size_t *lens,
               size_t n_shards, rse_stream_t stream);
/* encode_sep (core.rs:617-632) */
int rse_encode_sep(const rse_codec *codec, const void *const *data, const size_t *data_lens,
                   size_t n_data, void *const *parity, const size_t *parity_lens,
                   size_t n_parity, rse_stream_t stream);
/* encode_single (core.rs:545-562): i_data == 0 overwrites parity, later indices
 * accumulate (core.rs:503-507).  Used by ShardByShard (core.rs:101-231). */
int rse_encode_single(const rse_codec *codec, size_t i_data, void *const *shards,
                      const size_t *lens, size_t n_shards, rse_stream_t stream);
/* encode_single_sep (core.rs:576-592) */
int rse_encode_single_sep(const rse_codec *codec, size_t i_data, const void *single,
                          size_t single_len, void *const *parity, const size_t *parity_lens,
                          size_t n_parity, rse_stream_t stream);
/* verify (core.rs:637-651): *ok = 1 iff the parity matches.  Reads k+p shards
 * once, writes nothing.  Waits for the check (see above). */
int rse_verify(const rse_codec *codec, const void *const *shards, const size_t *lens,
               size_t n_shards, int *ok, rse_stream_t stream);
/* verify_with_buffer (core.rs:654-669): on RSE_OK the buffer holds the correct
 * parity whether or not verification passed (core.rs:328-331). */
int rse_verify_with_buffer(const rse_codec *codec, const void *const *shards,
                           const size_t *lens, size_t n_shards, void *const *buffer,
                           const size_t *buffer_lens, size_t n_buffer, int *ok,
                           rse_stream_t stream);
/* reconstruct / reconstruct_data (core.rs:680-695, 733-923) with the
 * ReconstructShard semantics of (T, bool) (lib.rs:168-200): present[i] != 0
 * marks shard i present; a missing shard's buffer must still have the common
 * length (else IncorrectShardSize) and is overwritten.  In data-only mode
 * missing parity buffers are neither checked nor touched (core.rs:805-806). */
int rse_reconstruct(const rse_codec *codec, void *const *shards, const size_t *lens,
                    const uint8_t *present, size_t n_shards, rse_stream_t stream);
int rse_reconstruct_data(const rse_codec *codec, void *const *shards, const size_t *lens,
                         const uint8_t *present, size_t n_shards, rse_stream_t stream);

/* ---- flat contiguous stripes (wasm/src/lib.rs:45-73 ABI, many stripes) --- */
/* `stripes` holds n_stripes consecutive stripes; each stripe is k+p shards of
 * shard_len elements laid end to end (the wasm encode() layout).  One launch. */
int rse_encode_flat(const rse_codec *codec, void *stripes, size_t shard_len,
                    size_t n_stripes, rse_stream_t stream);
/* verify (core.rs:637-651) of every stripe in one pass: ok[s] = 1 iff stripe
 * s's parity matches.  Reads each shard once, writes nothing.  Synchronises
 * `stream`.  (No reference counterpart: the crate verifies one stripe per
 * call; this is the batched form of the same check for scrubbing.) */
int rse_verify_flat(const rse_codec *codec, const void *stripes, size_t shard_len,
                    size_t n_stripes, uint8_t *ok, rse_stream_t stream);
/* Error LOCATION over the same layout: which shards of each stripe are wrong,
 * so that a scrub can repair what rse_verify_flat can only report.  (No
 * reference counterpart: the crate handles erasures only.)  The code is a
 * Reed-Solomon code of minimum distance p+1 (core.rs:430-436: every byte
 * column of a stripe is a polynomial of degree < k evaluated at 0..k+p-1), so
 * up to t = p/2 wrong shards per byte column are located exactly, by syndrome
 * decoding, in one pass that reads every shard once and writes only flags.
 * Per byte column: it is CLEAN if it is a codeword; DECODABLE if exactly one
 * codeword lies within Hamming distance t of it (its bad shards are where it
 * differs from that codeword); otherwise UNDECODABLE.  Per stripe s:
 *   every column clean                          status[s] = RSE_LOCATE_CLEAN,
 *                                               present row all 1;
 *   any column undecodable, or the union of bad shards over all columns has
 *   more than p members                         RSE_LOCATE_UNCORRECTABLE,
 *                                               present row all 1 (a
 *                                               reconstruct leaves it alone);
 *   otherwise                                   RSE_LOCATE_LOCATED, present 0
 *                                               exactly at the union, 1 elsewhere.
 * Different columns may have different bad shards: a union of more than t (up
 * to p) shards is still LOCATED as long as no single column needs more than t.
 * INHERENT LIMIT: a column with MORE than t wrong shards can lie within t of a
 * different codeword; it is then "decodable" and innocent shards are named.
 * Confirm a repair with rse_verify_flat.
 * present (n_stripes x (k+p) bytes) and status (n_stripes bytes) are DEVICE
 * memory of the stripes' device, written by kernels; stripes is only read.
 * Asynchronous on `stream`, no host synchronisation (the first call of a codec
 * on a device copies its plan there, once).  present can be handed unchanged
 * to rse_reconstruct_batch, which reads device flags in place.
 * Validation, before any device call, in this order: NULL codec / stripes /
 * present / status -> RSE_ERR_INVALID_ARGUMENT; a codec out of scope ->
 * RSE_ERR_INVALID_ARGUMENT (in scope: GF(2^8), 1 <= p <= 16, k + p <= 255;
 * GF(2^16) codecs, p > 16 and k + p = 256 are not supported, nor host memory);
 * shard_len == 0 -> RSE_EMPTY_SHARD; n_stripes == 0 -> RSE_OK, nothing touched.
 * Any shard_len >= 1 works, at whatever alignment the layout gives the shards. */
#define RSE_LOCATE_CLEAN 0         /* every column is a codeword */
#define RSE_LOCATE_LOCATED 1       /* bad shards named; at most p of them */
#define RSE_LOCATE_UNCORRECTABLE 2 /* some column is not within t = p/2 errors of a
                                      codeword, or more than p shards are implicated */
int rse_locate_flat(const rse_codec *codec, const void *stripes, size_t shard_len,
                    size_t n_stripes, uint8_t *present, uint8_t *status, rse_stream_t stream);
/* Error CORRECTION over the same layout, in place: the wrong bytes of every
 * stripe are repaired where they lie, in the one pass that finds them, and
 * known-missing shards (erasures) may be combined with unknown corruption.
 * (No reference counterpart.)  Same scope as rse_locate_flat.
 * present (nullable; n_stripes x (k+p) flags in DEVICE memory, read in place):
 * non-zero = present, 0 = erased, the convention of rse_reconstruct_batch and
 * of rse_locate_flat's output, so a locate result can be fed straight in.
 * NULL: nothing is erased.  An erased shard's buffer must exist; its contents
 * are arbitrary.  Let f be the number of erased shards of a stripe.
 * PER BYTE COLUMN (every byte column is its own codeword): the column is
 * DECODABLE when some codeword differs from it in nu positions outside the
 * erased set, and anywhere inside it, with 2 nu + f <= p; that codeword is
 * unique (minimum distance p+1).  A decodable column is overwritten with that
 * codeword -- only the bytes that differ are stored; an undecodable column is
 * left byte for byte as it was.  COLUMNS ARE INDEPENDENT: a stripe with an
 * undecodable column still gets its other columns repaired, and so may be
 * partly repaired when its status is RSE_CORRECT_UNCORRECTABLE.  A caller that
 * wants all-or-nothing per stripe runs rse_locate_flat first.  This also means
 * that a stripe whose columns implicate more than p shards between them, which
 * rse_locate_flat reports UNCORRECTABLE, is repaired here as long as no single
 * column needs more than its own 2 nu + f <= p.
 * If f > p the stripe is not touched at all (and not read).
 * INHERENT LIMIT: a column with more than (p-f)/2 errors may lie within reach
 * of another codeword; it is then decoded to that codeword.  Confirm with
 * rse_verify_flat.
 * Outputs, DEVICE memory of the stripes' device, written by kernels:
 *   status[s]      RSE_CORRECT_CLEAN / _CORRECTED / _UNCORRECTABLE (n_stripes);
 *   changed[s][r]  (nullable, n_stripes x (k+p)) 1 iff at least one byte of
 *                  shard r of stripe s was stored with a new value, else 0;
 *   counts[s]      (nullable, n_stripes x 2) {bytes stored, columns left
 *                  undecodable}; they saturate at 2^32-1 and never wrap; a
 *                  stripe skipped for f > p reports {0, 0}.
 * Asynchronous on `stream`, no host synchronisation (the codec's plan is
 * copied to a device once, the copy rse_locate_flat uses).
 * Validation, before any device call, in rse_locate_flat's order and with its
 * codes: NULL codec / stripes / status -> RSE_ERR_INVALID_ARGUMENT (present,
 * changed and counts may be NULL); a codec out of scope ->
 * RSE_ERR_INVALID_ARGUMENT; shard_len == 0 -> RSE_EMPTY_SHARD; n_stripes == 0
 * -> RSE_OK, nothing touched.  Any shard_len >= 1 works, at whatever alignment
 * the layout gives the shards. */
#define RSE_CORRECT_CLEAN 0          /* every column was a codeword; nothing written */
#define RSE_CORRECT_CORRECTED 1      /* every column is a codeword now */
#define RSE_CORRECT_UNCORRECTABLE 2  /* some column left as it was, or more than p shards erased
                                        (then nothing of the stripe is written) */
int rse_correct_flat(const rse_codec *codec, void *stripes, size_t shard_len, size_t n_stripes,
                     const uint8_t *present, /* nullable */
                     uint8_t *status,        /* n_stripes */
                     uint8_t *changed,       /* nullable, n_stripes x (k+p) */
                     uint32_t *counts,       /* nullable, n_stripes x 2 */
                     rse_stream_t stream);
/* Scrub: rse_correct_flat at the speed of rse_verify_flat where the stripes
 * are clean, and the list of those that were not.  `stripes`, `present`,
 * `status`, `changed` and `counts` are rse_correct_flat's, word for word: every
 * byte column decoded on its own, erasures beside errors with 2 nu + f <= p per
 * column, a stripe with f > p neither read nor written, saturating counts.  For
 * a codec both entries accept, those outputs and the stripe bytes after the
 * call equal rse_correct_flat's on the same input.
 *   n_bad        n_bad[0] = the number of stripes whose status is not
 *                RSE_CORRECT_CLEAN;
 *   bad_stripes  their indices in ascending order in bad_stripes[0 .. n_bad);
 *                entries from n_bad on are not written.
 * Either may be NULL alone.  All pointers but `codec` are device memory.
 * Codecs: rse_locate_flat's, and GF(2^16) codecs with 1 <= p <= 16 and
 * k + p <= 255 (their coefficients lie in the GF(2^8) subfield, so each byte of
 * each element is a GF(2^8) codeword of the same matrix; whatever
 * RSE_OPT_SUBFIELD says).  For those `shard_len` counts elements as everywhere
 * in this header, the decoder runs over 2 x shard_len bytes per shard, a byte
 * column is a column of bytes and counts[s][0] counts bytes.
 * Where the check of rse_verify_flat runs on bit-sliced or FFT kernels
 * (rse_codec_kernel_kind COMPILED, SPECIALISED or FFT; shards of 1 KiB, 2 KiB
 * or at least 4 KiB, 16-byte aligned) it runs first with its verdicts kept on
 * the device, and the repair pass visits only the stripes that failed it or
 * have an erased flag; otherwise the repair pass visits every stripe.  A codec
 * whose kernels are still being specialised is never waited for.
 * rse_last_kernel() names the route: "scrub gf8 10+4 prefilter" / "... direct".
 * Asynchronous on `stream`, no host synchronisation; every workspace is a
 * stream-ordered allocation of the call, so concurrent calls on different
 * streams share nothing.
 * Validation, before any device call, in this order: NULL codec / stripes /
 * status -> RSE_ERR_INVALID_ARGUMENT; a codec out of scope ->
 * RSE_ERR_INVALID_ARGUMENT; shard_len == 0 -> RSE_EMPTY_SHARD; n_stripes == 0
 * -> RSE_OK, nothing touched (n_bad neither); n_stripes > 2^32 - 1 ->
 * RSE_ERR_INVALID_ARGUMENT. */
int rse_scrub_flat(const rse_codec *codec, void *stripes, size_t shard_len, size_t n_stripes,
                   const uint8_t *present, /* nullable, n_stripes x (k+p) */
                   uint8_t *status,        /* n_stripes: RSE_CORRECT_* */
                   uint8_t *changed,       /* nullable, n_stripes x (k+p) */
                   uint32_t *counts,       /* nullable, n_stripes x 2 */
                   uint32_t *bad_stripes,  /* nullable, n_stripes */
                   uint32_t *n_bad,        /* nullable, 1 */
                   rse_stream_t stream);
/* rse_scrub_flat for shards that are allocated separately: one pointer per
 * shard, as rse_verify takes them, and a verdict per BLOCK of columns.
 *   shards, lens  HOST arrays of k + p entries; shards[i] is DEVICE memory, data
 *                 shards first and parity after; lens in elements, all equal.
 *                 The shards must not overlap (not checked).
 *   block_len     in elements; 0 = one block, the whole shard.  With
 *                 len = lens[0]: B = min(block_len, len) (len for 0) and
 *                 n_blocks = ceil(len / B).  Block b is elements
 *                 [b B, min((b+1) B, len)) of every shard: only the last block
 *                 may be shorter.
 * A block is to this entry what a stripe is to rse_scrub_flat, and every
 * sentence of that entry's contract holds with "block" for "stripe": every byte
 * column decoded on its own, erasures beside errors with 2 nu + f <= p per
 * column, a block with f > p neither read nor written, saturating counts, the
 * ascending list whose entries from n_bad on are not written, GF(2^16) codecs of
 * at most 255 shards decoded byte by byte.  `present` (nullable), `status`,
 * `changed`, `counts` (nullable), `bad_blocks` and `n_bad` (nullable, each
 * alone) are DEVICE memory with one row per block.  Defining property: the
 * bytes of block b and its rows of the outputs after the call equal those of
 * rse_scrub_flat run on the flat arrangement of block b alone, with shard_len =
 * that block's length and `present` row b.
 * Codecs: rse_scrub_flat's.  Routes: rse_scrub_flat's two, chosen once per
 * call by the same rule over the block's bytes and every pointer: the check
 * pass first where it runs on bit-sliced or FFT kernels now, B x element size is
 * 1 KiB, 2 KiB or at least 4 KiB and a multiple of 16, and every shards[i] is
 * 16-byte aligned; RSE_OPT_SCRUB_ROUTE forces either.  A shorter last block
 * follows the call's route.  The repair pass reads 16 bytes per lane only when
 * every shards[i] and the block's bytes are multiples of 16, else byte by byte.
 * rse_last_kernel(): "scrub-shards gf8 10+4 prefilter" / "... direct".
 * Asynchronous on `stream`, no host synchronisation; the host arrays are
 * consumed before the call returns; every workspace is a stream-ordered
 * allocation of the call.
 * Validation, before any device call, in this order: NULL codec / shards / lens
 * / status -> RSE_ERR_INVALID_ARGUMENT; a codec out of scope ->
 * RSE_ERR_INVALID_ARGUMENT; n_shards != k + p -> RSE_TOO_FEW_SHARDS /
 * RSE_TOO_MANY_SHARDS; lens[0] == 0 -> RSE_EMPTY_SHARD, unequal lens ->
 * RSE_INCORRECT_SHARD_SIZE; a NULL shards[i] -> RSE_ERR_INVALID_ARGUMENT;
 * n_blocks > 2^32 - 1 -> RSE_ERR_INVALID_ARGUMENT. */
int rse_scrub_shards(const rse_codec *codec, void *const *shards, const size_t *lens,
                     size_t n_shards, size_t block_len,
                     const uint8_t *present, /* nullable, DEVICE, n_blocks x (k+p) */
                     uint8_t *status,        /* DEVICE, n_blocks: RSE_CORRECT_* */
                     uint8_t *changed,       /* nullable, n_blocks x (k+p) */
                     uint32_t *counts,       /* nullable, n_blocks x 2 */
                     uint32_t *bad_blocks,   /* nullable, n_blocks */
                     uint32_t *n_bad,        /* nullable, 1 */
                     rse_stream_t stream);
/* Small writes: data shards of the flat layout rewritten in place, and the
 * parity patched by the delta instead of re-encoded.  `stripes` is
 * rse_encode_flat's layout.  Entry u of the list says: data shard
 * updates[2u+1] of stripe updates[2u] gets the shard_len elements at
 * new_data + u x shard_len x element size.  `new_data` is only read and must
 * not overlap `stripes` (not checked).
 * Effect, when the list is accepted: every named data shard holds its new
 * bytes, and in each touched stripe
 *     parity_j ^= sum_i M[k+j][i] x (old_i ^ new_i)
 * over that stripe's entries, for every parity row j (encode_single's
 * accumulation, core.rs:545-562, applied to a difference).  Nothing else is
 * written: no other data shard, no untouched stripe.  Defining property: the
 * syndrome of each touched stripe -- parity as stored XOR parity as re-encoded
 * from its data -- is what it was.  A stripe that verified before the call
 * verifies after it, with the parity of a fresh encode; a stripe with latent
 * corruption stays exactly as repairable by rse_scrub_flat as it was, where
 * re-encoding would have sealed the corruption into consistent parity.
 * Entry u is in order iff stripe_u < n_stripes, shard_u < k, and u == 0 or
 * (stripe_{u-1}, shard_{u-1}) < (stripe_u, shard_u) lexicographically on the
 * raw values: the list is strictly ascending, without duplicates, one stripe's
 * entries adjacent.
 *   result  required, 2 words.  Accepted: {RSE_UPDATE_APPLIED, the number of
 *           distinct stripes touched}.  Any entry not in order:
 *           {RSE_UPDATE_REJECTED, the index of the first such entry}, and not
 *           one byte of `stripes` is written; the call still returns RSE_OK (the
 *           host never reads the list).
 * `stripes`, `updates`, `new_data` and `result` are DEVICE memory.
 * Codecs: every GF(2^8) codec, k + p = 256 and any p included; GF(2^16) codecs
 * with k + p <= 256, byte by byte in the GF(2^8) subfield where their
 * coefficients lie (whatever RSE_OPT_SUBFIELD says; shard_len counts elements).
 * Out of scope: GF(2^16) codecs past 256 shards (RSE_ERR_INVALID_ARGUMENT),
 * host memory.  Separately allocated shards: rse_update_shards.  The read that
 * goes with these writes, while a shard is unavailable: rse_read_flat.
 * Any shard_len >= 1 at whatever alignment the layout gives: 16 bytes per lane
 * where `stripes`, `new_data` and shard_len x element size are all multiples
 * of 16, else byte by byte (correct, not fast).  rse_last_kernel() names the
 * route: "update gf8 10+4 vec" / "... bytes".
 * Traffic for p <= 16: 2 shard reads and 1 write per entry, p reads and p
 * writes per touched stripe; with p > 16 the entry's 2 reads are repeated for
 * every further 16 parity rows.  Measured (10+4, 512 stripes of 1 MiB shards,
 * MI355X): 0.98 ms for the parity of all 512 stripes plus 0.37 ms
 * per shard per stripe, at 4.4 TB/s of the traffic above.  One shard in every
 * 16th stripe: 0.11 ms against 1.40 ms for a device scatter and rse_encode_flat
 * over the batch.  The crossover against rse_encode_flat alone (1.34 ms) is one
 * shard in every stripe (1.35 ms); past it re-encoding is faster, 3.4 x with all
 * ten shards of every stripe written (4.67 ms) -- unless the syndrome matters.
 * Asynchronous on `stream`, no host synchronisation; two launches; every
 * workspace is a stream-ordered allocation of the call; it never requests or
 * waits for a run-time module.
 * Validation, before any device call, in this order: NULL codec / stripes /
 * updates / new_data / result -> RSE_ERR_INVALID_ARGUMENT; a codec out of scope
 * -> RSE_ERR_INVALID_ARGUMENT; shard_len == 0 -> RSE_EMPTY_SHARD; n_updates == 0
 * -> RSE_OK, nothing touched (result neither); n_stripes == 0, or n_stripes or
 * n_updates > 2^32 - 1 -> RSE_ERR_INVALID_ARGUMENT. */
#define RSE_UPDATE_APPLIED 0
#define RSE_UPDATE_REJECTED 1
int rse_update_flat(const rse_codec *codec, void *stripes, size_t shard_len, size_t n_stripes,
                    const uint32_t *updates, /* DEVICE, n_updates x 2: {stripe, data shard} */
                    const void *new_data,    /* DEVICE, n_updates x shard_len elements */
                    size_t n_updates,
                    uint32_t *result,        /* DEVICE, 2 words */
                    rse_stream_t stream);
/* rse_update_flat for shards that are allocated separately: one pointer per
 * shard and a cut into blocks of columns, both exactly as rse_scrub_shards takes
 * them, so a write touches a RANGE of a data shard.
 *   shards, lens  HOST arrays of k + p entries, consumed before the call
 *                 returns; shards[i] is DEVICE memory, data shards first; lens in
 *                 elements, all equal.
 *   block_len     in elements; 0 = one block.  With len = lens[0]:
 *                 B = min(block_len, len) (len for 0), n_blocks = ceil(len / B),
 *                 block b is elements [b B, min((b+1) B, len)) of every shard:
 *                 only the last block may be shorter.
 * A block is to this entry what a stripe is to rse_update_flat.  Entry u names
 * data shard updates[2u+1] of block updates[2u]; its new elements start at
 * new_data + u x B x element size -- rows always have stride B, and an entry for
 * the shorter last block uses the first elements of its row, as many as that
 * block has, the rest being ignored.  `new_data` is only read; it and the shards
 * must not overlap one another (not checked).  The in-order rule is
 * rse_update_flat's with n_blocks for n_stripes, and so is `result`:
 * {RSE_UPDATE_APPLIED, distinct blocks touched}, or {RSE_UPDATE_REJECTED, the
 * index of the first entry not in order} with not one shard byte written and
 * RSE_OK returned.  No address is formed from an entry that is not in order.
 * Defining property: the bytes of block b after the call equal those of
 * rse_update_flat run on the flat arrangement of block b alone, with shard_len =
 * that block's length, block b's entries in order and their rows of new_data.  A
 * block that no entry names keeps every byte, and so do bytes outside the
 * shards.  Each touched block's syndrome is what it was: write, update, scrub
 * (rse_scrub_shards, same shards and block_len) works in place.  The read that
 * goes with these writes, while a shard is unavailable or has no buffer:
 * rse_read_shards.
 * `updates`, `new_data` and `result` are DEVICE memory.
 * Codecs: rse_update_flat's.  Everything else, and shards, updates, new_data or
 * result in host memory: RSE_ERR_INVALID_ARGUMENT.
 * Route, chosen once per call: 16 bytes per lane where every shards[i],
 * `new_data`, B x element size and len x element size are all multiples of 16
 * (so the shorter last block is too), else byte by byte (correct at any length
 * and alignment, not fast).  rse_last_kernel(): "update-shards gf8 10+4 vec" /
 * "... bytes".
 * The kernel is rse_update_flat's with another address rule; the pointers
 * travel in its arguments (no device table, no copy).  Traffic as there.
 * Measured (10+4, 512 blocks of 1 MiB, MI355X): one shard in every
 * block 1.23 ms, in every 16th 0.10 ms, all ten in every block 4.21 ms, against
 * 1.28 / 0.09 / 4.50 ms for rse_update_flat on the same bytes laid flat and
 * 9.96 / 8.60 / 13.26 ms for gather, rse_update_flat, copy back.
 * Asynchronous on `stream`, no host synchronisation; two launches; the
 * workspace is a stream-ordered allocation of the call; it never requests or
 * waits for a run-time module.
 * Validation, before any device call, in this order: NULL codec / shards / lens
 * / updates / new_data / result -> RSE_ERR_INVALID_ARGUMENT; a codec out of scope
 * -> RSE_ERR_INVALID_ARGUMENT; n_shards != k + p -> RSE_TOO_FEW_SHARDS /
 * RSE_TOO_MANY_SHARDS; lens[0] == 0 -> RSE_EMPTY_SHARD, unequal lens ->
 * RSE_INCORRECT_SHARD_SIZE; a NULL shards[i] -> RSE_ERR_INVALID_ARGUMENT;
 * n_updates == 0 -> RSE_OK, nothing touched (result neither); n_blocks or
 * n_updates > 2^32 - 1 -> RSE_ERR_INVALID_ARGUMENT.  Then, with the device: a
 * pointer that is not device memory -> RSE_ERR_INVALID_ARGUMENT. */
int rse_update_shards(const rse_codec *codec, void *const *shards, const size_t *lens,
                      size_t n_shards, size_t block_len,
                      const uint32_t *updates, /* DEVICE, n_updates x 2: {block, data shard} */
                      const void *new_data,    /* DEVICE, n_updates x B elements */
                      size_t n_updates,
                      uint32_t *result,        /* DEVICE, 2 words */
                      rse_stream_t stream);
/* Degraded reads: shards of the flat layout read into a buffer of the
 * caller's, the erased ones rebuilt on the way.  `stripes` is rse_encode_flat's
 * layout and is only read.  Entry u of the list says: shard reads[2u+1] -- data
 * or parity -- of stripe reads[2u] goes to the shard_len elements at
 * out + u x shard_len x element size.  `out` must not overlap `stripes` (not
 * checked).  `present` is rse_reconstruct_batch's convention, n_stripes x
 * (k + p) flags, non-zero = present, row s for stripe s; NULL = every shard is
 * present.  The buffer of an erased shard must exist and is never read.
 * Effect, when the list is accepted, per entry:
 *   RSE_READ_COPIED   the shard is present: its bytes, copied.
 *   RSE_READ_REBUILT  the shard is erased and at least k shards of its stripe
 *                     are present: the bytes reconstruct (core.rs:733-923)
 *                     writes to it for that flag row.  The stripe's FIRST k
 *                     PRESENT SHARDS IN INDEX ORDER are the only inputs, missing
 *                     parity going through the rebuilt data.  On a stripe that
 *                     is not a codeword the choice of inputs decides the bytes,
 *                     so it belongs to the contract.
 *   RSE_READ_LOST     the shard is erased and fewer than k shards of its stripe
 *                     are present: the row keeps its bytes.  Present shards of
 *                     such a stripe are still copied.
 * Nothing else is written: no byte of `stripes`, no row past n_reads.
 * Rebuilding a failed device r onto a spare is the list {s, r} for every s.
 * Entry u is in order iff stripe_u < n_stripes, shard_u < k + p, and u == 0 or
 * (stripe_{u-1}, shard_{u-1}) < (stripe_u, shard_u) lexicographically on the
 * raw values: rse_update_flat's rule with k + p in the place of k.
 *   status  required, n_reads bytes: RSE_READ_COPIED / _REBUILT / _LOST.
 *   result  required, 2 words.  Accepted: {RSE_READ_SERVED, the number of
 *           entries whose status is RSE_READ_LOST}.  Any entry not in order:
 *           {RSE_READ_REJECTED, the index of the first such entry}; nothing of
 *           `out` or `status` is written, no address is formed from an entry
 *           out of order, and the call still returns RSE_OK (the host never
 *           reads the list).
 * `stripes`, `present`, `reads`, `out`, `status` and `result` are DEVICE memory.
 * Codecs: GF(2^8) codecs, and GF(2^16) codecs with k + p <= 256, both with
 * p <= 128 (the elimination of a stripe's plan is held in a workgroup's LDS as
 * bytes).  GF(2^16) codecs are coded byte by byte in the GF(2^8) subfield, where
 * their matrix lies and therefore its inverses too (whatever RSE_OPT_SUBFIELD
 * says; shard_len counts elements).  Everything else: RSE_ERR_INVALID_ARGUMENT.
 * Out of scope: host memory.  Separately allocated shards, and a shard that
 * has no buffer at all: rse_read_shards.
 * Any shard_len >= 1 at whatever alignment the layout gives: 16 bytes per lane
 * where `stripes`, `out` and shard_len x element size are all multiples of 16,
 * else byte by byte (correct at any length and alignment, not fast).
 * rse_last_kernel() names the route: "read gf8 10+4 vec" / "... bytes".
 * Traffic: a stripe's entries are served in groups of 16; per stripe and group
 * at most k shard reads (none where the group rebuilds nothing), and per entry
 * one write, plus one read if copied.  With more than 16 entries in a stripe
 * the valid set is read again for every further group.
 * Measured (10+4, 512 stripes of 1 MiB shards, MI355X), against
 * rse_reconstruct_batch(data_only = 1) over the batch with the same flags: one
 * erased data shard in every stripe, read: 1.36 ms, 4.4 TB/s of the traffic
 * above, against 1.14 ms -- slower beyond the run-to-run range, the table
 * multiply against the bit-sliced kernel; the same in every 16th stripe 0.13
 * against 0.15 ms; four erased shards per stripe 2.38 against 1.47 ms; one
 * present shard per stripe, a pure copy, 0.40 ms.  At 1 KiB shards x 65536
 * stripes, one erased shard per stripe: 1.33 against 1.43 ms, 0.56 TB/s; in every
 * 16th stripe 0.37 against 1.41 ms.
 * Asynchronous on `stream`, no host synchronisation; three launches (the list,
 * a plan per touched stripe, the read); every workspace is a stream-ordered
 * allocation of the call, 24 bytes per entry and data shard; it never requests
 * or waits for a run-time module.
 * Validation, before any device call, in this order: NULL codec / stripes /
 * reads / out / status / result -> RSE_ERR_INVALID_ARGUMENT; a codec out of
 * scope -> RSE_ERR_INVALID_ARGUMENT; shard_len == 0 -> RSE_EMPTY_SHARD;
 * n_reads == 0 -> RSE_OK, nothing touched (result neither); n_stripes == 0, or
 * n_stripes or n_reads > 2^32 - 1 -> RSE_ERR_INVALID_ARGUMENT. */
#define RSE_READ_SERVED 0
#define RSE_READ_REJECTED 1
#define RSE_READ_COPIED 0   /* the shard is present: its bytes, copied */
#define RSE_READ_REBUILT 1  /* rebuilt from the stripe's first k present shards */
#define RSE_READ_LOST 2     /* fewer than k shards of the stripe are present: row not written */
int rse_read_flat(const rse_codec *codec, const void *stripes, size_t shard_len, size_t n_stripes,
                  const uint8_t *present, /* nullable, DEVICE, n_stripes x (k+p) */
                  const uint32_t *reads,  /* DEVICE, n_reads x 2: {stripe, shard}, shard < k + p */
                  size_t n_reads,
                  void *out,              /* DEVICE, n_reads x shard_len elements */
                  uint8_t *status,        /* DEVICE, n_reads: RSE_READ_COPIED / _REBUILT / _LOST */
                  uint32_t *result,       /* DEVICE, 2 words */
                  rse_stream_t stream);
/* rse_read_flat for shards that are allocated separately: one pointer per
 * shard and a cut into blocks of columns, both exactly as rse_scrub_shards and
 * rse_update_shards take them, so an entry reads a RANGE of a shard.  The shards
 * are only read.
 *   shards, lens  HOST arrays of k + p entries, consumed before the call
 *                 returns; shards[i] is DEVICE memory or NULL (below), data
 *                 shards first; lens in elements, all equal.
 *   block_len     in elements; 0 = one block.  With len = lens[0]:
 *                 B = min(block_len, len) (len for 0), n_blocks = ceil(len / B),
 *                 block b is elements [b B, min((b+1) B, len)) of every shard:
 *                 only the last block may be shorter.
 * A block is to this entry what a stripe is to rse_read_flat.  Entry u names
 * shard reads[2u+1] -- data or parity -- of block reads[2u]; its row starts at
 * out + u x B x element size -- rows always have stride B, and an entry of the
 * shorter last block writes the first elements of its row, as many as that
 * block has, the rest of the row keeping its bytes.  `out` must not overlap the
 * shards (not checked).  `present` is n_blocks x (k + p) flags, non-zero =
 * present, row b for block b; NULL = every shard that has a buffer is present.
 * The in-order rule is rse_read_flat's with n_blocks for n_stripes, and so are
 * `status` and `result`: {RSE_READ_SERVED, the number of RSE_READ_LOST entries},
 * or {RSE_READ_REJECTED, the index of the first entry not in order} with nothing
 * of `out` or `status` written, no address formed from an entry out of order,
 * and RSE_OK returned.
 * A shard without a buffer: shards[i] == NULL declares shard i erased in EVERY
 * block, whatever `present` says and also where `present` is NULL -- a failure
 * domain that is down has nothing to point at.  No address is ever formed from
 * it: it is never in a block's valid set and never RSE_READ_COPIED; its entries
 * are RSE_READ_REBUILT or RSE_READ_LOST.  Any number of shards may be NULL; with
 * more than p of them every erased entry is RSE_READ_LOST and the present shards
 * are still copied.  lens[i] of such a shard must still equal the others.
 * Rebuilding a failed device r onto a spare: shards[r] = NULL, the list {b, r}
 * for every b, `out` the spare (with B = block_len dividing len, or one block).
 * Defining property: entry {b, r}'s row (the block's own length of it) and its
 * `status` equal those of rse_read_flat run on the flat arrangement of block b
 * alone, with shard_len = that block's length and flag row b with the flags of
 * the NULL shards cleared; result[1] counts the RSE_READ_LOST entries.  Nothing
 * of `out` past what the entries' blocks cover is written, and no shard byte.
 * `present`, `reads`, `out`, `status` and `result` are DEVICE memory.
 * Codecs: rse_read_flat's.  Everything else, and a non-NULL shards[i], present,
 * reads, out, status or result in host memory: RSE_ERR_INVALID_ARGUMENT.
 * Route, chosen once per call: 16 bytes per lane where every non-NULL
 * shards[i], `out`, B x element size and len x element size are all multiples
 * of 16 (so the shorter last block and every row are too), else byte by byte
 * (correct at any length and alignment, not fast).  rse_last_kernel():
 * "read-shards gf8 10+4 vec" / "... bytes".
 * The kernels are rse_read_flat's: the same list pass, the same planner with
 * the pointer table as its "has no buffer" predicate, the read kernel with
 * another address rule; the pointers travel in the kernels' arguments (no
 * device table, no copy).  Traffic as there.
 * Measured (10+4, 512 blocks of 1 MiB, MI355X): one erased shard in
 * every block 1.35 ms, in every 16th 0.12 ms, one present shard per block 0.38
 * ms, four erased per block 2.39 ms, one shard without a buffer read whole 1.35
 * ms, against 1.32 / 0.12 / 0.37 / 2.35 / 1.32 ms for rse_read_flat on the same
 * bytes laid flat -- 2 to 3 % slower, within the run-to-run range except with
 * four per block -- and 5.55 / 4.35 / 4.62 / 6.59 / 5.27 ms for gather, then
 * rse_read_flat.
 * Asynchronous on `stream`, no host synchronisation; three launches; the
 * workspace is a stream-ordered allocation of the call; it never requests or
 * waits for a run-time module.
 * Validation, before any device call, in this order: NULL codec / shards / lens
 * / reads / out / status / result -> RSE_ERR_INVALID_ARGUMENT; a codec out of
 * scope -> RSE_ERR_INVALID_ARGUMENT; n_shards != k + p -> RSE_TOO_FEW_SHARDS /
 * RSE_TOO_MANY_SHARDS; lens[0] == 0 -> RSE_EMPTY_SHARD, unequal lens ->
 * RSE_INCORRECT_SHARD_SIZE; n_reads == 0 -> RSE_OK, nothing touched (result
 * neither); n_blocks or n_reads > 2^32 - 1 -> RSE_ERR_INVALID_ARGUMENT.  A NULL
 * shards[i] is not refused.  Then, with the device: a pointer that is not
 * device memory -> RSE_ERR_INVALID_ARGUMENT. */
int rse_read_shards(const rse_codec *codec, const void *const *shards, const size_t *lens,
                    size_t n_shards, size_t block_len,
                    const uint8_t *present, /* nullable, DEVICE, n_blocks x (k+p) */
                    const uint32_t *reads,  /* DEVICE, n_reads x 2: {block, shard}, shard < k + p */
                    size_t n_reads,
                    void *out,              /* DEVICE, n_reads x B elements */
                    uint8_t *status,        /* DEVICE, n_reads: RSE_READ_COPIED / _REBUILT / _LOST */
                    uint32_t *result,       /* DEVICE, 2 words */
                    rse_stream_t stream);
/* rse_encode_flat's layout; every stripe has the same erasure pattern `present[k+p]`
 * (wasm reconstruct(): reconstruct_data semantics). */
int rse_reconstruct_data_flat(const rse_codec *codec, void *stripes, size_t shard_len,
                              size_t n_stripes, const uint8_t *present, rse_stream_t stream);
/* Same layout; EVERY stripe has its own erasure pattern: present is
 * n_stripes x (k+p) flags, row s for stripe s.  reconstruct (data_only = 0,
 * core.rs:680) or reconstruct_data (data_only = 1, core.rs:690) of each stripe,
 * with the per-stripe planning of core.rs:733-923 (valid/invalid partition,
 * decode-matrix inversion, composed parity rows) done by a HIP kernel: two
 * launches for the whole batch.  Errors (TooFewShardsPresent / EmptyShard for
 * the first offending stripe) are detected before any stripe is modified.
 * Whole 16 KiB chunks of codecs with bit-sliced kernels (compiled in or run-time
 * specialised, either field) are planned per stripe on the device (e x e
 * syndrome inverse) and coded by the bit-sliced syndrome kernel; the rest of
 * every shard, and other GF(2^8) codecs with k <= 32 and p <= 16, use the
 * device planner with k x k inverses and the table kernels; anything else
 * falls back to the host planner stripe by stripe (same results).  `present`
 * may be host memory or device memory of the stripes' device (flags a GPU
 * scrub produced: they are then read in place, never copied, and the
 * shared-pattern detection -- a host pass -- is skipped).  Returns after the
 * work is queued and the host inputs have been consumed.  To read named shards
 * of degraded stripes into another buffer, the stripes left as they are:
 * rse_read_flat. */
int rse_reconstruct_batch(const rse_codec *codec, void *stripes, size_t shard_len,
                          size_t n_stripes, const uint8_t *present, int data_only,
                          rse_stream_t stream);

/* ---- low level: the fused kernel itself ------------------------------ */
/* outputs[r] (+)= sum_i rows[r*n_in + i] * inputs[i] over len elements.
 * rows is HOST memory, n_out x n_in elements (GF(2^16): [u8;2] each).
 * accumulate = 0 reproduces code_some_slices (core.rs:481-490, first input
 * overwrites); accumulate = 1 XORs into the outputs (mul_slice_add). */
int rse_code_shards(int field, const uint8_t *rows, size_t n_out, size_t n_in,
                    const void *const *inputs, void *const *outputs, size_t len,
                    int accumulate, rse_stream_t stream);
/* rse_code_shards on HOST inputs and outputs (the host pipeline above): the
 * one hook that puts the reference's code_some_slices (core.rs:481-490) on
 * the GPU unchanged -- encode, verify and reconstruct all funnel into it
 * (core.rs:522, 629, 861, 918).  Synchronous. */
int rse_code_shards_host(int field, const uint8_t *rows, size_t n_out, size_t n_in,
                         const void *const *inputs, void *const *outputs, size_t len,
                         int accumulate, rse_stream_t stream);
/* The Field/FFI slice hooks below take in/out WHEREVER THEY LIVE, as the
 * reference's callers do (they pass host slices): the library asks the runtime
 * (hipPointerGetAttributes) where each buffer is.
 *  - in and out both device memory of one device (hipMalloc, managed): the
 *    kernel, asynchronous on `stream`;
 *  - either in host memory (pageable, pinned or registered): the host
 *    pipeline -- H2D, kernel, D2H -- synchronous: out holds the result on
 *    return.  Pinned memory overlaps the copies; pageable memory works.
 * galois_8 mul_slice / mul_slice_xor (galois_8.rs:291-327): out = c*in (or
 * out ^= c*in) over GF(2^8). */
int rse_gf8_mul_slice(uint8_t c, const void *in, void *out, size_t len, int xor_into,
                      rse_stream_t stream);
/* The reference FFI kernel itself, same signature and contract:
 * reedsolomon_gal_mul / reedsolomon_gal_mul_xor (simd_c/reedsolomon.h:30-42,
 * bound at galois_8.rs:267-283).  low/high are the coefficient's 16-entry
 * nibble tables (MUL_TABLE_LOW/HIGH[c], build.rs:75-94; host memory); in/out
 * host or device memory as above.  Returns when out holds the result, as the
 * CPU kernel does, having waited only for its own work (a library stream, not
 * the whole device).  Returns the bytes processed: len (no scalar tail for
 * the caller to finish, galois_8.rs:301-304), or 0 on a device failure with
 * nothing written (rse_last_device_error says why).  On host slices a 0 lets
 * the reference's tail loop do the whole slice on the CPU, which is correct;
 * a caller passing DEVICE slices must treat 0 (for len > 0) as an error and
 * never run a host tail on them. */
size_t rse_gal_mul(const uint8_t *low, const uint8_t *high, const uint8_t *in, uint8_t *out,
                   size_t len);
size_t rse_gal_mul_xor(const uint8_t *low, const uint8_t *high, const uint8_t *in, uint8_t *out,
                       size_t len);
/* galois_16's Field::mul_slice / mul_slice_add (the trait defaults,
 * lib.rs:99-118), host or device memory as above: c is one [u8;2] element
 * {coefficient of x, constant}; len counts elements.  add_into = 0:
 * out = c*in, 1: out += c*in. */
int rse_gf16_mul_slice(const uint8_t *c, const void *in, void *out, size_t len, int add_into,
                       rse_stream_t stream);

/* ---- device matrix inversion (matrix.rs:195-261 semantics) ----------- */
/* Invert `batch` n x n matrices (device memory, row-major), one workgroup per
 * matrix (Gauss-Jordan; the augmented matrix in LDS up to n = 127, else in a
 * stream-ordered device workspace).  singular[b] = 1 for a singular matrix
 * (matrix.rs:11-13 Error::SingularMatrix; its out[b] is left unwritten), else
 * 0.  Asynchronous on `stream`.
 * GF(2^8): one byte per element, n <= 255 (the field's largest codec). */
int rse_gf8_invert_batch(const void *d_in, void *d_out, uint32_t *d_singular, size_t n,
                         size_t batch, rse_stream_t stream);
/* GF(2^16): [u8;2] elements {coefficient of x, constant} (galois_16.rs:49-51),
 * n <= 4096.  The decode matrices of galois_16 codecs (core.rs:697-731). */
int rse_gf16_invert_batch(const void *d_in, void *d_out, uint32_t *d_singular, size_t n,
                          size_t batch, rse_stream_t stream);

/* ---- host-memory (end-to-end) path ----------------------------------- */
/* The reference API's own form: shards are caller slices in HOST memory
 * (core.rs:597-695).  Each call pipelines chunks of every shard through the
 * device -- H2D of the shards the operation reads, the kernels, D2H of the
 * shards it writes, on separate streams over a ring of device buffers -- and
 * returns when the results are in host memory (synchronous).  Only what the
 * operation needs crosses PCIe: reconstruct uploads the k valid shards of
 * core.rs:801-841 and downloads only the rebuilt ones.  Pinned host memory
 * gives overlapped DMA; pageable memory works but serialises the copies.
 * Same validation, error precedence and results as the device entries. */
/* encode (core.rs:597-611) */
int rse_encode_host(const rse_codec *codec, void *const *shards, const size_t *lens,
                    size_t n_shards, rse_stream_t stream);
/* encode_sep (core.rs:617-632), encode_single (core.rs:545-562) and
 * encode_single_sep (core.rs:576-592; ShardByShard's calls) on host shards. */
int rse_encode_sep_host(const rse_codec *codec, const void *const *data, const size_t *data_lens,
                        size_t n_data, void *const *parity, const size_t *parity_lens,
                        size_t n_parity, rse_stream_t stream);
int rse_encode_single_host(const rse_codec *codec, size_t i_data, void *const *shards,
                           const size_t *lens, size_t n_shards, rse_stream_t stream);
int rse_encode_single_sep_host(const rse_codec *codec, size_t i_data, const void *single,
                               size_t single_len, void *const *parity, const size_t *parity_lens,
                               size_t n_parity, rse_stream_t stream);
/* Flat host stripes (rse_encode_flat layout, HOST memory): the same pipeline
 * over every chunk of every stripe, so PCIe stays busy across stripes. */
int rse_encode_host_flat(const rse_codec *codec, void *stripes, size_t shard_len,
                         size_t n_stripes, rse_stream_t stream);
/* verify (core.rs:637-651) / verify_with_buffer (core.rs:654-669; the host
 * buffer receives the correct parity on RSE_OK) */
int rse_verify_host(const rse_codec *codec, const void *const *shards, const size_t *lens,
                    size_t n_shards, int *ok, rse_stream_t stream);
int rse_verify_with_buffer_host(const rse_codec *codec, const void *const *shards,
                                const size_t *lens, size_t n_shards, void *const *buffer,
                                const size_t *buffer_lens, size_t n_buffer, int *ok,
                                rse_stream_t stream);
/* rse_verify_flat over flat HOST stripes: ok[s] per stripe. */
int rse_verify_host_flat(const rse_codec *codec, const void *stripes, size_t shard_len,
                         size_t n_stripes, uint8_t *ok, rse_stream_t stream);
/* reconstruct / reconstruct_data (core.rs:680-695) with (T, bool) semantics,
 * as rse_reconstruct / rse_reconstruct_data. */
int rse_reconstruct_host(const rse_codec *codec, void *const *shards, const size_t *lens,
                         const uint8_t *present, size_t n_shards, rse_stream_t stream);
int rse_reconstruct_data_host(const rse_codec *codec, void *const *shards, const size_t *lens,
                              const uint8_t *present, size_t n_shards, rse_stream_t stream);
/* rse_reconstruct_batch over flat HOST stripes: every stripe its own erasure
 * pattern (present: n_stripes x (k+p)); stripes with nothing missing move no
 * bytes.  Errors are detected before any stripe is touched. */
int rse_reconstruct_host_batch(const rse_codec *codec, void *stripes, size_t shard_len,
                               size_t n_stripes, const uint8_t *present, int data_only,
                               rse_stream_t stream);

/* ---- synchronous calls (the reference's own contract) ----------------- */
/* encode / verify / reconstruct / reconstruct_data of ONE stripe of device
 * shards that return when the result is in device memory, like the
 * reference's ReedSolomon methods (core.rs:597-611, 637-651, 680-695): same
 * validation, errors and bytes as rse_encode / rse_verify / rse_reconstruct /
 * rse_reconstruct_data.  No stream: the call is not ordered after work the
 * caller queued -- the caller has finished writing the shards it passes (for
 * example by synchronising its stream).  Small stripes (GF(2^8) codecs and
 * GF(2^16) codecs of at most 256 shards, 16-byte aligned shards, at most
 * RSE_OPT_DISPATCH_MAX_BYTES per shard, k x outputs <= 1024) go to a resident
 * workgroup that polls pinned host memory for requests (RSE_OPT_DISPATCH): no
 * kernel launch, no stream synchronisation -- a round trip of a few
 * microseconds.  It ends by itself after RSE_OPT_DISPATCH_IDLE_US without a
 * call, so it never holds the device for longer (a hipDeviceSynchronize may
 * wait that long).  Anything else runs the usual kernels on a library stream
 * and waits for them.  Thread-safe; calls to one device are served one at a
 * time. */
int rse_encode_now(const rse_codec *codec, void *const *shards, const size_t *lens, size_t n);
int rse_verify_now(const rse_codec *codec, const void *const *shards, const size_t *lens,
                   size_t n, int *ok);
int rse_reconstruct_now(const rse_codec *codec, void *const *shards, const size_t *lens,
                        const uint8_t *present, size_t n);
int rse_reconstruct_data_now(const rse_codec *codec, void *const *shards, const size_t *lens,
                             const uint8_t *present, size_t n);
/* Ends the resident dispatcher kernels now (they end by themselves when idle). */
void rse_dispatcher_stop(void);

/* ---- options (rse_set_option / rse_get_option) --------------------------
 * The options a caller of the drop-in may set: run-time specialisation, the
 * host pipeline, the resident dispatcher; and read-only counters.  Results
 * never depend on any option.  The library's tuning and A/B switches (launch
 * shapes, kernel variants, network generators; include/rse_hip_tune.h) are
 * refused with RSE_ERR_INVALID_ARGUMENT unless the environment has
 * RSE_TUNE=1 (the test suite and tools/ set it). */
#define RSE_OPT_BITSLICE_LAUNCHES 6 /* read-only, per thread: number of bit-sliced kernel
                                       launches so far (diagnostics / tests) */
#define RSE_OPT_HOST_CHUNK_KIB 7    /* rse_*_host*: bytes per shard per pipeline chunk, KiB */
#define RSE_OPT_HOST_H2D_STREAMS 8  /* rse_*_host*: streams carrying H2D copies (1..4) */
#define RSE_OPT_JIT 9               /* run-time specialised kernels: 0 off, 1 used once built
                                       (default), 2 the first launch waits for the build */
#define RSE_OPT_JIT_MODULES 10      /* read-only: specialised modules compiled by this process
                                       (builds run in rse_jitc helper processes, several at a
                                       time, when the helper sits next to the library) */
#define RSE_OPT_JIT_PATTERNS 11     /* 1: decode patterns used twice get their own specialised
                                       kernel (reconstruct at encode speed); 0 off */
#define RSE_OPT_PATTERN_LAUNCHES 12 /* read-only, per thread: reconstructs that ran on a
                                       decode-pattern kernel */
#define RSE_OPT_JIT_DISK_CACHE 15   /* 1 (default): specialised modules are cached on disk
                                       ($RSE_JIT_CACHE_DIR, else $XDG_CACHE_HOME/rse_hip, else
                                       ~/.cache/rse_hip), keyed by library version + source, so
                                       another process loads them instead of compiling */
#define RSE_OPT_JIT_CACHE_HITS 16   /* read-only: modules this process loaded from the disk cache */
#define RSE_OPT_SCRATCH_LIVE 24     /* read-only: per-call device resource sets (verdict words, library
                                       stream, host-pipeline streams/events/ring) in existence, leased or
                                       idle.  Calls lease one from a process-wide pool that keeps at most 4
                                       idle per device, so threads that come and go leave nothing behind */
#define RSE_OPT_HOST_PLANNED_STRIPES 25 /* read-only, per thread: stripes rse_reconstruct_batch
                                       planned on the host (a batch past the device planner's LDS
                                       budget: more than 8192 shards or very many erasures) */
#define RSE_OPT_JIT_MAX_PATTERNS 35  /* decode-pattern modules built per process (default 64);
                                        past it, patterns run on the syndrome / table kernels */
#define RSE_OPT_JIT_MAX_PATTERN_BLOCKS 36 /* blocks of wide decode patterns per process (64) */
#define RSE_OPT_DISPATCH 39           /* 1 (default): small *_now calls run on the resident dispatcher;
                                        0: always the launch path (A/B) */
#define RSE_OPT_DISPATCH_IDLE_US 40   /* the resident dispatcher ends after this many microseconds
                                        without a call (default 200).  It runs on a low-priority
                                        stream, so other streams' kernels never queue behind it,
                                        but a device-wide synchronisation (hipDeviceSynchronize,
                                        torch.cuda.synchronize()) right after a *_now call waits
                                        until it has idled out: ~230 us per call+sync at 200,
                                        ~2 ms at 2000 (tools/dispatch_sync_probe.py);
                                        rse_dispatcher_stop() ends it at once */
#define RSE_OPT_DISPATCH_MAX_BYTES 41 /* shard bytes up to which a *_now call is dispatched
                                        (default 65536) */
#define RSE_OPT_DISPATCHED 42         /* read-only: *_now calls the dispatcher served */
#define RSE_OPT_DISPATCH_LAUNCHES 43  /* read-only: launches of the resident dispatcher */
#define RSE_OPT_DISPATCH_WORKGROUPS 45 /* workgroups of the resident dispatcher (1..64, default 8):
                                        a request is coded by as many as its size needs; only
                                        the first polls more than 16 bytes per poll. Read at launch */
/* Process-wide; returns RSE_ERR_INVALID_ARGUMENT for an unknown key, a refused value, or a
 * tuning key without RSE_TUNE=1. */
int rse_set_option(int key, int64_t value);
/* Current value, or -1 for an unknown key. */
int64_t rse_get_option(int key);

/* ---- utilities (benchmarks and tests) -------------------------------- */
/* Fill device memory with the splitmix64 byte stream of (seed, shard_id):
 * 64-bit word w = mix(seed + shard_id * 2^40 + w), little endian. */
int rse_fill_splitmix(void *dst, size_t nbytes, uint64_t seed, uint64_t shard_id,
                      rse_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSE_HIP_H */
