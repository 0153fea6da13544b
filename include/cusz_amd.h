/* include/cusz_amd.h -- extensions of this implementation beyond the cuSZ C API.
 *
 * None of these exist in the reference; they expose what the MI355X build measures and
 * what the parity tests need (stage timings, intermediate device buffers, tuning knobs,
 * slab sharding helpers for multi-GPU runs).  All functions return the status codes below.
 */
#ifndef CUSZ_AMD_EXT_H
#define CUSZ_AMD_EXT_H

#ifdef __cplusplus
extern "C" {
#endif

#include <stddef.h>
#include <stdint.h>

#include "cusz/context.h"

/* Status codes.  Every entry point returns a psz_error_status value (cusz/type.h: the reference's
 * values, used where one applies: PSZ_ABORT_UNSUPPORTED_TYPE for a dtype mismatch,
 * PSZ_ABORT_UNSUPPORTED_DIMENSION for an archive of another shape, ...) or one of these, for
 * failures the reference enum has no value for (it reports them as crashes or exceptions): */
#define PSZ_AMD_ERR_INVALID_ARG 100 /* null handle or pointer, a size or knob value out of range   */
#define PSZ_AMD_ERR_BAD_ARCHIVE 101 /* archive or header malformed, truncated or inconsistent      */
#define PSZ_AMD_ERR_DEVICE 102      /* a HIP runtime call, allocation or kernel launch failed       */
#define PSZ_AMD_ERR_STATE 103       /* call out of order (compress_finish without a pending scan)   */
#define PSZ_AMD_ERR_ENCODER 104     /* the encoder's own overflow / look-back check failed (a bug)  */
#define PSZ_AMD_ERR_CODE_RANGE 105  /* spline: a quantisation code the archive cannot carry, below  */

/* The spline predictor's domain.  A point whose code leaves [0, 2 radius) is stored as an outlier
 * cell {f32 code, u32 index} (the reference's format), and the compressor predicts the following
 * points from the exact code.  Compress (psz_compress_*, and psz_amd_compress_finish after a scan)
 * returns PSZ_AMD_ERR_CODE_RANGE, and hands back no archive pointer, when
 *   - double fields: some outlier's code is not a float, i.e. |prediction error| / (2 eb) beyond
 *     2^24 (up to rounding: codes that a float holds exactly pass), or
 *   - either dtype: |prediction error| / (2 eb) reaches 2^31 - 1024 (code + radius must stay an
 *     int; an infinite value does so too, a NaN has no defined result with any predictor).
 * float fields between 2^24 and that limit are accepted: both sides compute with the
 * float-rounded code, and the error is one float ulp of the value.  Use a larger bound, or the
 * Lorenzo predictor (its cells hold values, not codes). */

/* Stage indices for psz_amd_stage_times (milliseconds of the last call, HIP events on the
 * manager's stream; only filled after psz_amd_enable_timing(m, 1)). */
enum {
  PSZ_AMD_T_EXTREMA = 0,   /* Rel mode range probe                         */
  PSZ_AMD_T_PREDICT = 1,   /* Lorenzo predict-quantize + histogram + outliers */
  PSZ_AMD_T_BOOK = 2,      /* histogram D2H + host codebook + H2D (FZG: 0)  */
  PSZ_AMD_T_ENCODE = 3,    /* Huffman encode (bit packing + look-back); FZG: its three launches */
  PSZ_AMD_T_FINALIZE = 4,  /* outlier compaction + headers + readback       */
  PSZ_AMD_T_COMPRESS = 5,  /* whole compress call                           */
  PSZ_AMD_T_SCATTER = 6,   /* decompress: outlier scatter (+ zeroing)       */
  PSZ_AMD_T_DECODE = 7,    /* decompress: Huffman decode; FZG: its decode launch */
  PSZ_AMD_T_RECON = 8,     /* decompress: Lorenzo reconstruct               */
  PSZ_AMD_T_DECOMPRESS = 9,/* whole decompress call                         */
  PSZ_AMD_T_COUNT = 10
};

typedef struct psz_amd_internals {
  uint16_t* d_quant_codes; /* quant codes of the last compress (or decoded codes) */
  uint32_t* d_hist;        /* histogram u32[bklen] of the last compress          */
  uint32_t* d_book;        /* codebook u32[bklen]                                 */
  size_t len;              /* number of elements                                  */
  int bklen;
  int sublen;
  int pardeg;
  int ndim;
  size_t splen;            /* outlier cells of the last compress                  */
  size_t archive_capacity; /* bytes reserved for the device archive               */
  int layout;              /* archive layout of the last compress: PSZ_AMD_LAYOUT_* */
  int brick_width;         /* chunk length of the brick layout (0: not eligible)  */
} psz_amd_internals;

int psz_amd_get_internals(psz_resource* m, psz_amd_internals* out);
int psz_amd_enable_timing(psz_resource* m, int on);
int psz_amd_stage_times(psz_resource* m, float* ms, int n);

/* Override the Huffman chunk length (symbols per chunk, rounded up to a multiple of 256,
 * at most 8192) used by the next compress; 0 restores the default (nCU * 512 chunks, see
 * DESIGN.md; the reference's libphf.cc:26-70 rule targets one encode thread per chunk). */
int psz_amd_set_sublen(psz_resource* m, int sublen);

/* Decode-only entry point used by the multi-GPU gather path and tests: decodes the Huffman
 * segment of a device archive into the manager's code buffer. */
int psz_amd_decode_codes(psz_resource* m, uint8_t* IN_d_compressed);

/* Huffman decoder selection: 0 auto (default: the fused brick decoder when the archive's chunk
 * length is the brick width, else lane/wave by chunk count), 1 one lane per chunk
 * (LDS-windowed), 2 one wave per chunk.  1 and 2 decode into the code buffer and reconstruct
 * separately.  All decode the same archives bit-exactly; tests exercise each.  Other values
 * are rejected. */
#define PSZ_AMD_DECODER_AUTO 0
#define PSZ_AMD_DECODER_LANE 1
#define PSZ_AMD_DECODER_WAVE 2
int psz_amd_set_decoder(psz_resource* m, int kind);

/* Archive layout.  Both are the reference phf format (chunk c of sublen codes at par_entry[c]).
 *  BRICK (default when eligible: 3-D, x extent a multiple of the brick width): chunk = one brick
 *    row, predictor fused with the encoder and decoder with the reconstructor; chunks are laid
 *    out brick by brick with zero cells between brick regions.
 *  REFERENCE: chunks in index order, no gaps (byte-identical to the reference encoder). */
#define PSZ_AMD_LAYOUT_BRICK 0
#define PSZ_AMD_LAYOUT_REFERENCE 1
/* BRICK_FORCE: the brick layout also for small 2-D fields (BRICK keeps the reference layout for
 * 2-D fields with fewer than 4 bricks per CU, where it is faster). */
#define PSZ_AMD_LAYOUT_BRICK_FORCE 2
int psz_amd_set_layout(psz_resource* m, int layout);

/* Codebook source.  Quant codes, outliers, the error bound and the decompressed field are the
 * same in every mode; the codebook (hence the bitstream and, marginally, the CR) differs.  Every
 * archive is an ordinary phf archive: the reference decoder reads it.
 *  EXACT: the reference's codebook (its binary heap, hf_bk_impl1.seq.cc) of the full histogram,
 *    built on the host (compressor.inl:339-458): the archive is byte-identical to the reference
 *    encoder's output for the same codes and chunking.
 *  SAMPLED (default): no host round trip on the critical path.  3-D and 1-D brick fields: pass 1
 *    visits every 33rd brick first (17th / 9th / 5th / 3rd / all for fewer bricks) and hands that
 *    sample's histogram to the host mid-pass, which builds the two-queue Huffman codebook of
 *    sample + 1 per bin while pass 1 goes on (the device builder's algorithm, run on the host).
 *    Reference layout and 2-D bricks: the EXACT book of the full histogram (published by the
 *    predictor's last workgroup).  Spline fields and a sharded finish (reduced histogram): the
 *    two-queue codebook of the full histogram built on the DEVICE (book_device.hh; the same
 *    total bits as the heap's on the same histogram).
 *  STREAM (3-D brick fields): the sampled codebook, then ONE pass predicts and packs (k_brick3_
 *    stream: no code buffer, no gaps between bricks); experimental. */
#define PSZ_AMD_CODEBOOK_EXACT 0
#define PSZ_AMD_CODEBOOK_SAMPLED 1
#define PSZ_AMD_CODEBOOK_STREAM 2
int psz_amd_set_codebook(psz_resource* m, int mode);

/* ---- the FZG codec: psz_pipeline.codec1 = FZCodec (cusz/type.h; `cusz --codec fzgcodec`) ----
 * A second lossless stage for callers who prefer throughput to ratio: no histogram, no codebook, no
 * host round trip, nothing data-dependent serial.  Lorenzo and LorenzoZigZag, 1-D to 3-D, f32 and
 * f64; Spline with FZCodec returns PSZ_ABORT_NO_SUCH_CODEC, as every codec but Huffman and FZCodec
 * does.  The quant codes, the outlier cells, the error bound and the decompressed field are those
 * of the Huffman path; only the segment at entry[PSZHEADER_ENCODED] differs.  The reference ships a
 * codec of this family without wiring it into its pipeline, so there is no reference format to
 * match: this one is this build's own, and the archive is a pure function of the codes.
 *
 * Format.  Symbols are the u16 codes in index order, as they are (LorenzoZigZag, transform 0) or
 * as zigzag(code - radius) (Lorenzo, transform 1: small deltas of either sign keep only low bits,
 * the outlier code 0 becomes 2 radius - 1).  A unit is 256 consecutive symbols: lane l of 64 holds
 * symbols 4l..4l+3 as one little-endian u64, and word w (0..63) of the unit has bit l = bit w of
 * lane l's u64 (a 64 x 64 bit transpose).  The unit's flag has bit w set iff word w is nonzero; its
 * payload is its nonzero words in ascending w.  Symbols past the field's end count as 0.
 *   segment = u32 magic "FZG1" | u32 unit = 256 | u32 transform | u32 units | u32 blocks | u32 0
 *             | u64 payload words                                                 (32 bytes)
 *           | u64 flags[units]
 *           | u32 block_off[blocks + 1]: payload words before each block of 16 units (4096
 *             symbols), [blocks] = the total; padded to 8 bytes
 *           | u64 payload[words], unit after unit, no gaps
 * psz_header: pipeline.codec1 = FZCodec, vle_sublen = 4096, vle_pardeg = blocks, entry[] and splen
 * as for Huffman; the outlier cells follow the segment.  Worst case: 2 bytes a symbol + 1/32 +
 * 1/1024; the manager's archive capacity covers it.
 *
 * Decompression reads the codec from the header.  Before anything is queued the segment is
 * checked (the header's entries on the host; the segment's 32-byte header and last offset in one
 * small synchronous read-back, the only host wait): magic, unit size, unit and block counts
 * against the field, the segment inside the archive, offsets and payload inside the segment.  A
 * violation returns PSZ_AMD_ERR_BAD_ARCHIVE with nothing launched and nothing written.  Corrupt
 * flags or offsets inside a well-formed segment give wrong values, never a read outside it.  The
 * archive pointer must be 8-byte aligned (PSZ_AMD_ERR_INVALID_ARG otherwise).
 *
 * What does not apply: psz_amd_set_sublen / _decoder / _layout / _codebook are accepted and have
 * no effect on an FZG compress or decompress (the codes always take the reference layout;
 * psz_amd_internals.layout says so).  psz_amd_compress_scan_* still exports the histogram; of the
 * histogram passed to psz_amd_compress_finish only the overflow word counts.  Stage times:
 * PSZ_AMD_T_BOOK is 0, PSZ_AMD_T_ENCODE / _DECODE are the FZG kernels.  Region decode takes
 * PSZ_AMD_REGION_FALLBACK (psz_amd_region_plan says so), or PSZ_AMD_REGION_SLAB over the covering
 * blocks in PSZ_AMD_REGION_MODE_COVER.  psz_amd_merge_archives returns
 * PSZ_ABORT_NO_SUCH_CODEC for FZG parts. */

/* ---- sharded compress (multi-GPU; the reference has no multi-GPU path) ----
 * A field split into tile-aligned slabs (z: multiples of 8 planes) is compressed one slab per
 * GPU with ONE codebook:
 *   1. psz_amd_compress_scan_*: pass 1 only (predict, histogram, outliers); the slab's
 *      histogram u32[2 * radius] is copied to OUT_d_hist (device, on the manager's stream),
 *      followed by one more word: the slab's outlier cells beyond its current capacity.
 *   2. the caller sums these u32[2 * radius + 1] of all slabs (e.g. an RCCL all-reduce).
 *   3. psz_amd_compress_finish: codebook from IN_d_hist (device u32[2 * radius + 1]; NULL: the
 *      slab's own histogram), encode, archive -- outputs as psz_compress_float.  When the last
 *      word is nonzero (some slab had more outliers than its capacity: past the reference's
 *      10 %), every slab's finish returns PSZ_WARN_OUTLIER_TOO_MANY, the slabs that overflowed
 *      have grown their capacity, and repeating steps 1-3 succeeds on every rank together.
 *      IN_d_hist must count every symbol this slab uses: a bin that is 0 where the slab's own
 *      pass-1 histogram is not (a sum over slabs cannot be; a wrong reduction can) would leave a
 *      used symbol without a codeword, so the finish returns PSZ_AMD_ERR_INVALID_ARG, leaves
 *      OUT_d_compressed and OUT_compressed_bytes untouched and consumes the pending scan; the
 *      manager stays usable (scan again, finish with the right histogram).  Any other relation
 *      between the two histograms is accepted -- counts smaller than the slab's own included,
 *      as long as they are nonzero.  The check runs on the device and costs no host wait; FZG
 *      archives, which use no codebook, are exempt, spline archives are not.
 * psz_compress_analyize_float (cusz_rev1.h) is step 1 with the histogram exported to the host
 * (compressor.inl:305-337). */
int psz_amd_compress_scan_float(psz_resource* m, psz_rc2 rc, float* IN_d_data, uint32_t* OUT_d_hist);
int psz_amd_compress_scan_double(psz_resource* m, psz_rc2 rc, double* IN_d_data, uint32_t* OUT_d_hist);
int psz_amd_compress_finish(psz_resource* m, const uint32_t* IN_d_hist, psz_header* OUT_header,
                            uint8_t** OUT_d_compressed, size_t* OUT_compressed_bytes);

/* Value range of a device field of the manager's dtype and length: writes {min, max} as two
 * doubles to OUT_d_minmax (device memory), queued on the manager's stream (no host sync).  The
 * Rel (r2r) mode probe of libcusz.cc:287-293 / extrema.cuhip.inl:150-208, exported so that a
 * sharded compress can all-reduce the slabs' ranges before pass 1.  IN_len = 0 means the
 * manager's length. */
int psz_amd_value_range(psz_resource* m, const void* IN_d_data, size_t IN_len, double* OUT_d_minmax);

/* Merge per-slab archives (HOST memory, in field order) compressed with one shared codebook
 * into the archive of the whole field: the archive one process would have written for it
 * (chunks concatenated, par_entry rebased by the cells before each slab, outlier indices by
 * the slab's element offset).  elem_offsets (may be NULL) are checked against the running
 * sum.  *out_bytes receives the merged size; with out == NULL that is all (a size query,
 * PSZ_SUCCESS); with out_cap too small nothing is written and PSZ_AMD_ERR_INVALID_ARG is
 * returned.  Malformed parts: PSZ_AMD_ERR_BAD_ARCHIVE; parts that are not tile-aligned slabs of
 * the field: PSZ_ABORT_UNSUPPORTED_DIMENSION; parts of different runs (codebook, eb, dtype):
 * PSZ_AMD_ERR_INVALID_ARG / PSZ_ABORT_UNSUPPORTED_TYPE. */
int psz_amd_merge_archives(const uint8_t* const* parts, const size_t* part_bytes, int nparts,
                           const size_t* elem_offsets, psz_len full_len, uint8_t* out, size_t out_cap,
                           size_t* out_bytes);

/* ---- region-of-interest decompression (the reference reconstructs whole fields only) ----
 * Decode the box of `extent` elements at `origin` (both in elements, any alignment, extent >= 1
 * per axis; unused axes: origin 0, extent 1) of an archive of the manager's whole field into
 * OUT_d_box, a compact device array of extent.x * extent.y * extent.z elements (x fastest).  It
 * need not be zeroed and nothing outside it is written.  The result is bit-identical to the same
 * box of psz_decompress_*.  Header, length, dtype and archive checks are those of
 * psz_decompress_* (PSZ_ABORT_UNSUPPORTED_TYPE, PSZ_AMD_ERR_BAD_ARCHIVE, ...); a box that is
 * empty or leaves the field: PSZ_AMD_ERR_INVALID_ARG, nothing written.
 *  FUSED: 3-D brick-eligible fields (x a multiple of the brick width 256), Lorenzo, chunk length
 *    256, default decoder, outlier cells in this compressor's order: only the 256 x 8 x 8 bricks
 *    that cover the box are decoded, each whole (64 Huffman chunks), and only the box is stored.
 *  FALLBACK: everything else (1-D, 2-D, other shapes or chunk lengths, ZigZag, Spline, cells in
 *    another order, a forced LANE / WAVE decoder): the whole field is decompressed into a scratch
 *    field the manager allocates on first use, and the box copied out.  Correct everywhere, not
 *    fast.
 *  FUSED, 1-D (only in PSZ_AMD_REGION_MODE_COVER, below): 1-D brick-layout archives (Lorenzo,
 *    Huffman, chunk length 256, one chunk per 256 elements, 2 radius <= 1024), default decoder,
 *    cells in index order: only the tiles of 1024 elements that cover the range are decoded and
 *    reconstructed in one kernel, and only the range is stored.  Here the brick fields count
 *    TILES OF 1024 ELEMENTS: brick_lo = {t0, 0, 0}, brick_n = {t1 - t0, 1, 1}, bricks = t1 - t0
 *    with t0 = origin.x / 1024 and t1 = ceil((origin.x + extent.x) / 1024); chunks = min(4 t1,
 *    the archive's chunks) - 4 t0.
 *  SLAB (only in PSZ_AMD_REGION_MODE_COVER, below): every Lorenzo / LorenzoZigZag archive, Huffman
 *    or FZG, that is not FUSED.  Lorenzo prediction restarts at every tile, so only the slab of
 *    whole tiles along the slowest axis that covers the box is decoded: [a, b) with a = floor(o /
 *    T) T and b = min(len, ceil((o + e) / T) T), where T is 8 planes (3-D), 32 rows (2-D) or 1024
 *    elements (1-D) and o, e the box's origin and extent on that axis.  The Huffman chunks (FZG:
 *    the blocks of 4096) that hold the slab's codes are decoded, the slab's outlier cells
 *    scattered (in any order), the slab reconstructed in a scratch of its own size and the box
 *    copied out: time and memory follow the slab, not the field.
 * The work is queued on the manager's stream.  When the archive has outlier cells, a FUSED
 * candidate waits once for a 4-byte read-back (are the cells in brick order?) before its decode
 * is queued; no other host synchronisation.  Like psz_decompress_*, a region call invalidates a
 * pending psz_amd_compress_scan_*. */
#define PSZ_AMD_REGION_FUSED 0
#define PSZ_AMD_REGION_FALLBACK 1
#define PSZ_AMD_REGION_SLAB 2
typedef struct psz_amd_region_info {
  int path;                  /* PSZ_AMD_REGION_FUSED, _FALLBACK or _SLAB                      */
  psz_len brick_lo, brick_n; /* covering brick box: first brick, bricks per axis (FUSED), else zeros */
  size_t bricks;             /* bricks decoded (1-D FUSED: tiles of 1024; FALLBACK, SLAB: 0)  */
  size_t chunks;             /* Huffman chunks decoded (FUSED: 64 per brick; FALLBACK: all;
                              * SLAB: the chunks, or FZG blocks, that cover the slab)         */
  size_t elems;              /* extent.x * extent.y * extent.z                                */
} psz_amd_region_info;

/* How a manager decodes a region of an archive that is no FUSED candidate.
 *  WHOLE (the default): FALLBACK, exactly as before the mode existed.
 *  COVER: FUSED for 1-D brick-layout archives, SLAB for every other Lorenzo archive; a FUSED
 *    candidate (1-D or 3-D) that the device-side checks refuse
 *    (a forced decoder, cells in another order) takes SLAB too.  Spline and unknown codecs keep
 *    FALLBACK, as does an archive whose chunk length is no multiple of 8 (none this compressor
 *    writes).  The bits of the box are the same in either mode.
 * Other values: PSZ_AMD_ERR_INVALID_ARG, the mode stays. */
#define PSZ_AMD_REGION_MODE_WHOLE 0
#define PSZ_AMD_REGION_MODE_COVER 1
int psz_amd_set_region_mode(psz_resource* m, int mode);

/* Host only, no GPU: validates the box against the header's field and says what a region decode
 * of such an archive touches.  The path is the header's verdict; the device-side checks (the
 * manager's decoder knob, the cells' order) can still turn FUSED into FALLBACK (COVER: SLAB): see
 * psz_amd_last_region.  psz_amd_region_plan is psz_amd_region_plan_mode with
 * PSZ_AMD_REGION_MODE_WHOLE; a mode that is neither: PSZ_AMD_ERR_INVALID_ARG. */
int psz_amd_region_plan(const psz_header* h, psz_len origin, psz_len extent, psz_amd_region_info* out);
int psz_amd_region_plan_mode(const psz_header* h, psz_len origin, psz_len extent, int mode, psz_amd_region_info* out);

int psz_amd_decompress_region_float(psz_resource* m, uint8_t* IN_d_compressed, size_t IN_bytes, psz_len origin,
                                    psz_len extent, float* OUT_d_box);
int psz_amd_decompress_region_double(psz_resource* m, uint8_t* IN_d_compressed, size_t IN_bytes, psz_len origin,
                                     psz_len extent, double* OUT_d_box);
/* What the last successful region call on this manager did (the path taken after the device-side
 * checks); PSZ_AMD_ERR_STATE before the first one. */
int psz_amd_last_region(psz_resource* m, psz_amd_region_info* out);

/* ---- quality assessment on the device (the reference's GPU_assess_quality, GPU_find_max_error,
 * GPU_error_bounded and GPU_identical, psz/include/detail/compare.hh, in one pass) ----
 * Fills the reference's psz_statistics (cusz/type.h) for a reconstruction x against an original o,
 * both device arrays of len elements of the suffix's type, each read once.  o and x are converted
 * to double (exact), e_i = |x_i - o_i| is one double operation, and everything in `stat` runs
 * over the finite pairs (both values finite; m = n_finite of them):
 *   odata / xdata: min, max, rng = max - min, avg, std = sqrt(sum (v - avg)^2 / m)
 *   max_err_abs = max e_i; max_err_idx = the lowest index that attains it (a region call: an index
 *     into the compact box); max_err_rel = max_err_abs / odata.rng;
 *     max_err_pwrrel = max e_i / |o_i| over o_i != 0 (NaN when there is none)
 *   score_MSE = sum e^2 / m; score_NRMSE = sqrt(MSE) / odata.rng;
 *     score_PSNR = 20 log10(odata.rng) - 10 log10(MSE)
 *   score_coeff = (sum (o - avg_o)(x - avg_x) / m) / (std_o std_x)
 *   user_eb = eb, len = len
 *   autocor_lag_k (k = one, two): with PSZ_AMD_QUALITY_AUTOCOR the same correlation between
 *     o[0 .. len - k) and o[k .. len) over their finite pairs; NaN without the flag or when none.
 * Degenerate inputs take what IEEE gives: MSE 0 makes PSNR +inf, a zero std makes the coefficient
 * NaN, n_finite == 0 makes every double of stat NaN (user_eb aside) and the indices SIZE_MAX.
 * xdata.max is the reconstruction's and the error is kept in double (the reference's CPU path,
 * compare.stl.inl:89 and :92, takes the former from odata and rounds the latter to float).
 *
 * Means, variances and the covariance come from per-lane shifted sums combined pairwise (Chan et
 * al.), never from sum v^2 / n - mean^2; no floating-point atomics: two calls on the same inputs
 * return byte-identical structs.
 *
 * The manager supplies the stream and a scratch buffer for partial records, allocated on the first
 * quality call (never by compress or decompress).  len is any value >= 1, whatever the manager's
 * field and dtype; the pointers need element alignment only.  The call queues on the manager's
 * stream, waits once for the result and writes OUT_host.  It only reads: a pending
 * psz_amd_compress_scan_* stays valid.  PSZ_AMD_ERR_INVALID_ARG, OUT_host untouched: a null handle
 * or pointer, len == 0, eb negative or NaN, unknown flag bits, an empty box or one that leaves
 * the field. */
#define PSZ_AMD_QUALITY_AUTOCOR 1 /* also fill autocor_lag_one / _two (else NaN) */

typedef struct psz_amd_quality {
  psz_statistics stat;        /* the reference's struct, every field filled */
  size_t n_finite;            /* pairs with both values finite: everything in stat is over these */
  size_t n_nonfinite;         /* len - n_finite */
  size_t n_unbounded;         /* pairs with |x - o| > 1.001 * eb (the reference's CPU_error_bounded rule),
                                 plus non-finite pairs whose bit patterns differ; 0 when eb == 0 */
  size_t first_unbounded_idx; /* lowest such index, SIZE_MAX when none */
  size_t first_diff_idx;      /* lowest index whose bit patterns differ (GPU_identical), SIZE_MAX when identical */
} psz_amd_quality;

int psz_amd_assess_quality_float(psz_resource* m, const float* IN_d_xdata, const float* IN_d_odata, size_t len,
                                 double eb, int flags, psz_amd_quality* OUT_host);
int psz_amd_assess_quality_double(psz_resource* m, const double* IN_d_xdata, const double* IN_d_odata, size_t len,
                                  double eb, int flags, psz_amd_quality* OUT_host);
/* A compact box (what psz_amd_decompress_region_* wrote: extent elements, x fastest) against the
 * same box of the whole original field of field_len elements.  Indices and the autocorrelation are
 * those of the box as one array of extent.x * extent.y * extent.z elements. */
int psz_amd_assess_quality_region_float(psz_resource* m, const float* IN_d_xbox, const float* IN_d_ofield,
                                        psz_len field_len, psz_len origin, psz_len extent, double eb, int flags,
                                        psz_amd_quality* OUT_host);
int psz_amd_assess_quality_region_double(psz_resource* m, const double* IN_d_xbox, const double* IN_d_ofield,
                                         psz_len field_len, psz_len origin, psz_len extent, double eb, int flags,
                                         psz_amd_quality* OUT_host);
/* Host only: the statistics of a field from those of its consecutive parts (the slabs of a sharded
 * run), parts[i] starting at element elem_offsets[i] = the sum of the lengths before it
 * (PSZ_AMD_ERR_INVALID_ARG otherwise, and for parts of different user_eb).  Each part's record is
 * rebuilt from its n_finite, avg, std, score_coeff and score_MSE and combined as the kernel
 * combines; indices are moved by the offsets, ties go to the lowest index.  The autocorrelations
 * of a field do not follow from those of its parts: they are NaN. */
int psz_amd_quality_merge(const psz_amd_quality* parts, const size_t* elem_offsets, int nparts,
                          psz_amd_quality* out);

const char* psz_amd_version(void);

/* The device codebook (no host round trip; NOT the reference's heap order, the same total bit
 * count): canonical Huffman book (u32[bklen]) and reverse book (4 * 64 + 2 * bklen bytes) of the
 * device histogram IN_d_hist (+ smooth per bin: 1 makes every symbol encodable), all device
 * pointers, on `stream`.  bklen <= 1024.  Spline fields, sharded finishes and the stream mode build
 * their book this way. */
int psz_amd_build_book_device(const uint32_t* IN_d_hist, int bklen, uint32_t smooth, uint32_t* OUT_d_book,
                              uint8_t* OUT_d_revbook, void* stream);

/* Status of this thread's last psz_create_resource_manager* call (PSZ_SUCCESS when it returned a
 * manager): the resource-manager API returns NULL on failure, as the reference does, and this
 * says why -- e.g. PSZ_ABORT_UNSUPPORTED_DIMENSION for a shape the build does not take. */
int psz_amd_last_create_status(void);

#ifdef __cplusplus
}
#endif

#endif /* CUSZ_AMD_EXT_H */
