// cusz_amd/csrc/kernels.hh -- launchers of the hand-written gfx950 kernels.
#pragma once

#include "archive_layout.hh"
#include "common.hh"
#include "region_cover.hh"

namespace cusz_amd {

struct XferRegions {
  int count;
  int nwords[4];
  uint32_t* dst[4];
  const uint32_t* src[4];
};
// Words the last workgroup of a kernel copies to the host before raising a host flag (the
// kernel's own publish: no separate launch; pub_device.hh publish_last).  ticket: 9 words zeroed
// before the launch.
struct HostPub {
  XferRegions r{};
  uint32_t* flag = nullptr;  // null: no publish
  uint32_t epoch = 0;
  uint32_t* ticket = nullptr;
};

// Brick decomposition of the Lorenzo kernels (one wave64 per brick).
struct LorenzoGeom {
  int ndim;
  int V;                  // elements per lane along x
  uint32_t nbx, nby, nbz; // bricks per axis
  uint32_t nbricks;
  uint32_t brick_elems;   // elements per full brick
};

LorenzoGeom lorenzo_geom(int ndim, size_t lx, size_t ly, size_t lz, int elem_bytes);

template <typename T>
int launch_lorenzo_c(const T* in, size_t lx, size_t ly, size_t lz, double eb, int radius, bool zigzag,
                     const LorenzoGeom& g, uint16_t* codes, const OutlierSink& ol, uint32_t* hist,
                     int bklen, hipStream_t st, const HostPub& pub = HostPub{});

// The archive's outlier cells as the reconstructing kernels read them: straight from the archive,
// grouped by brick, when a bounds pass found them in order; otherwise (*unsorted == epoch) the
// scatter pass (launch_scatter with only_if = unsorted) has written the values into `out`, which
// the kernels read instead.
//  * 1-D Lorenzo (non-ZigZag): cells in strictly increasing index order (this compressor's
//    archives without spill).  Code 0 marks exactly the outliers, so the k-th zero code of a
//    brick takes the brick's k-th cell.  Bounds: launch_x1d_bounds.
//  * the fused brick decoders: cells grouped by brick and sorted by (row, x) (this compressor
//    writes them so); the decoder ranks the zero codes of each row against the brick's cells.
//    Bounds: launch_brick_cell_bounds (3-D), launch_x1d_bounds over chunks (1-D).
struct BrickOutliers {
  const uint32_t* cells = nullptr;  // archive cells {f32 value, u32 idx}
  size_t ncell = 0;
  const uint32_t* bstart = nullptr;    // nbricks + 1
  const uint32_t* unsorted = nullptr;  // == epoch: unsorted (the flag word is never reset)
  uint32_t epoch = 0;
};
// bstart over units of 2^ushift elements (16384: the 1-D reconstruction; 256: 1-D brick chunks)
int launch_x1d_bounds(const uint32_t* cells, size_t ncell, size_t n, uint32_t nbricks, uint32_t* bstart,
                      uint32_t* unsorted, uint32_t epoch, hipStream_t st, uint32_t ushift = 14);

template <typename T>
int launch_lorenzo_x(const uint16_t* codes, T* out, size_t lx, size_t ly, size_t lz, double eb, int radius,
                     bool zigzag, const LorenzoGeom& g, hipStream_t st, const BrickOutliers* ox = nullptr);

template <typename T>
int launch_scatter(const uint32_t* cells, size_t nnz, T* out, size_t n, hipStream_t st,
                   const uint32_t* only_if = nullptr, uint32_t epoch = 0);

// ---- Huffman, reference layout (hf_encode.hip, hf_decode.hip) -------------------------------
struct HfEncodeArgs {
  const uint16_t* codes;
  size_t n;
  const uint32_t* book;  // device u32[bklen]
  int bklen;
  int sublen;            // multiple of 256, <= 8192
  int pardeg;
  uint32_t* par_nbit;    // archive segment
  uint32_t* par_entry;   // archive segment
  uint32_t* bitstream;   // archive segment (4-byte aligned)
  uint32_t* temp;              // scratch of hf_encode_temp_words()
  uint32_t* ticket;            // kPubTicketWords words zeroed per call (the tile-sum launch's last workgroup
                               // scans up to 2,048 tiles itself)
  unsigned long long* total_nbit = nullptr;  // if set: the tile-sum pass writes the sum of every chunk's bits
};
int launch_hf_encode(const HfEncodeArgs& a, hipStream_t st);
size_t hf_encode_temp_words(int sublen, int pardeg);

// decode table scratch (u32 words): L1 4096 | maxl | first[] | bases | L2 2048, then a 32-B
// sink the lane decoder stores to when it has nothing to flush
constexpr int kHfDecTableWords = 4096 + 128 + 2048;
constexpr int kHfDecScratchWords = kHfDecTableWords + 16;

// The one chooser of the decoders that write codes in index order (chunk c's at codes[sublen c ...]):
// the chunk decoder (launch_chunk_decode) when the knob is AUTO and it can read the archive, else
// the LANE window decoder or the WAVE decoder (hf_decode.hip, which states the rule).
// lut: scratch u32[kHfDecScratchWords], 16-B aligned; decoder: PSZ_AMD_DECODER_*; ncu: the device's CUs
int launch_hf_decode(const PhfView& v, size_t n, uint16_t* codes, uint32_t* lut, int decoder, int ncu,
                     hipStream_t st);

// ---- FZG codec (fzg.hip): bit-plane shuffle + zero-word coder, archive_layout.hh FzgLayout ----
// symbols: the codes (transform kFzgPlain) or zigzag(code - radius) (kFzgZigzagDelta)
struct FzgEncodeArgs {
  const uint16_t* codes;  // index order, 8-byte aligned
  size_t n;
  int radius;
  uint32_t transform;
  uint64_t* flags;        // segment sections (8-byte aligned)
  uint32_t* block_off;
  uint64_t* payload;
  CompressInfo* info;     // total_ncell <- the payload in 4-byte cells (two a word)
};
// sizing (flags, words per block) -> one-workgroup scan (block_off, total) -> packing
int launch_fzg_encode(const FzgEncodeArgs& a, hipStream_t st);
struct FzgDecodeArgs {
  const uint64_t* flags;
  const uint32_t* block_off;
  const uint64_t* payload;
  uint64_t total_words;   // loads at or past it read 0 (a corrupt flag or offset stays inside the archive)
  size_t n;
  int radius;
  uint32_t transform;
  uint16_t* codes;        // 8-byte aligned
};
int launch_fzg_decode(const FzgDecodeArgs& a, hipStream_t st);

// ---- pipeline glue (pipeline_kernels.hip) ---------------------------------------------------
struct FinalizeArgs {
  // Huffman
  const uint32_t* par_nbit;
  const uint32_t* par_entry;
  int pardeg;
  // outliers
  const uint32_t* brick_cnt;
  uint32_t nbricks;
  uint32_t cap_per_brick;
  const uint32_t* spill_cnt;
  uint32_t spill_cap;
  uint32_t* brick_off;  // scratch u32[nbricks+1]
  CompressInfo* info;
  const uint32_t* spill_start = nullptr;  // OutlierSink::spill_start (ranged spill) or nullptr
  bool sizes_known = false;  // brick path: total_nbit / total_ncell already in info (reservation)
  bool nbit_known = false;   // info->total_nbit already summed (the encoder's tile-sum pass)
};
// psz_tpl / phf_tpl non-null: the same workgroup also writes both headers (no separate launch).
// fzg: phf_tpl is an FzgHeader, phf_offset / bitstream_rel its segment's offset and its payload's,
// and info->total_ncell the payload in 4-byte cells (sizes_known)
int launch_finalize_scan(const FinalizeArgs& a, hipStream_t st, const void* psz_tpl = nullptr,
                         const void* phf_tpl = nullptr, uint8_t* archive = nullptr, size_t phf_offset = 0,
                         size_t bitstream_rel = 0, bool fzg = false);

struct OutlierCopyArgs {
  const uint64_t* slots;
  const uint32_t* brick_cnt;
  const uint32_t* brick_off;
  uint32_t nbricks;
  uint32_t cap_per_brick;
  const uint64_t* spill;
  const uint32_t* spill_cnt;
  uint32_t spill_cap;
  const CompressInfo* info;
  uint8_t* archive;         // base of the archive
  size_t bitstream_offset;  // byte offset of the bitstream (outliers follow it)
  const uint32_t* spill_start = nullptr;  // OutlierSink::spill_start (ranged spill) or nullptr
};
int launch_outlier_copy(const OutlierCopyArgs& a, hipStream_t st, const HostPub& pub = HostPub{});


// small host<->device transfers through host-mapped pinned memory (no stream sync)
int launch_publish(const XferRegions& r, uint32_t* flag, uint32_t epoch, hipStream_t st);
int launch_upload(const XferRegions& r, hipStream_t st);
// upload behind a device-polled host gate (the host sets *gate = epoch when the data is ready)
int launch_gate_upload(const XferRegions& r, const uint32_t* gate, uint32_t epoch, unsigned int* timeout,
                       hipStream_t st);
int launch_zero(const XferRegions& r, hipStream_t st);  // dst/nwords only
// device codebook (book_device.hh): one workgroup, histogram (+ smooth per bin) -> book + revbook
int launch_book_device(const uint32_t* hist, int bklen, uint32_t smooth, uint32_t* book, uint8_t* revbook,
                       hipStream_t st);
int launch_excess(const uint32_t* spill_cnt, uint32_t cap, uint32_t* dst, hipStream_t st);
// a caller's histogram (bklen counts + the overflow word) over the scan's own, in place; a bin the
// caller left 0 that the scan counted takes weight 1 and raises *missing
int launch_take_hist(const uint32_t* ext, uint32_t* hist, int bklen, unsigned int* missing, hipStream_t st);

// ---- cuSZ-i spline3 (spline.hip) -----------------------------------------------------------
struct SplineGeom {
  uint32_t gdx, gdy, gdz, ntiles;  // 32 x 8 x 8 tiles (spline3.cu:29)
  size_t anchor_len;               // ceil(x/8) * ceil(y/8) * ceil(z/8) (buf_comp.cc:35-43)
};
SplineGeom spline_geom(size_t x, size_t y, size_t z);

template <typename T>
struct SplineArgs {
  const T* in;
  uint32_t X, Y, Z;
  uint32_t gdx, gdy, gdz, ntiles;
  float eb_r, ebx2;  // (float)(1/eb), (float)(2 eb): compressor.inl:107-108, FP = float
  int radius;
  int bklen;
  uint16_t* codes;
  T* anchor;      // anchor_len values (written into the archive's anchor segment)
  OutlierSink ol; // one slot range per tile (cap_per_brick), spill list beyond
  uint32_t* hist;
  uint32_t* code_lost;  // set when an outlier cell cannot carry its code (zeroed per call)
};
template <typename T>
int launch_spline3_c(const SplineArgs<T>& a, hipStream_t st);

template <typename T>
struct SplineXArgs {
  const uint16_t* codes;
  const T* anchor;
  T* out;
  uint32_t X, Y, Z;
  uint32_t gdx, gdy, gdz, ntiles;
  float eb_r, ebx2;
  int radius;
  const uint32_t* boff = nullptr;     // per-tile bucket offsets (set by the launcher)
  const uint32_t* bucket = nullptr;   // outlier cells {code bits, idx} grouped by tile (unsorted archives)
  const uint32_t* cells = nullptr;    // the archive's cells (already grouped: archives of this compressor)
  const uint32_t* unsorted = nullptr; // device flag: use `bucket` instead of `cells`
  size_t nbucket = 0;
  // outlier index -> (x, y, z) by multiply-high: q = mulhi(i, m) >> s for divisors X and Y
  // (set by the launcher; exact for i < 2^31; ndiv = true makes the kernel divide instead)
  uint32_t mX = 0, sX = 0, mY = 0, sY = 0;
  bool ndiv = true;
};
// cells: the archive's outlier segment ({f32 code, u32 idx} each); scratch: spline_x_scratch_words
template <typename T>
int launch_spline3_x(SplineXArgs<T> a, const uint32_t* cells, size_t ncell, uint32_t* scratch, hipStream_t st);
size_t spline_x_scratch_words(uint32_t ntiles, size_t ncell);

// ---- fused brick pipeline (brick_scan / brick_pack / brick_stream / brick3_decode / brick1_decode /
// chunk_decode .hip) ----------------------------------------------------------------------------
// A wave owns a W x 8 x 8 brick (W = 64 V); the Huffman chunk length equals W so each brick row
// is one chunk.  Eligible: 3-D with lx % W == 0, and 1-D (a brick = 64 consecutive chunks, 16
// tiles of 1024; the last brick and chunk may be short).
struct BrickGeom {
  bool ok;
  int ndim;
  int V, W;
  uint32_t nbx, nby, nbz, nbricks;
  uint32_t brick_elems;
  uint32_t nchunks;
  size_t n;
};
BrickGeom brick_geom(int ndim, size_t lx, size_t ly, size_t lz, int elem_bytes);

struct BrickLaunch {
  BrickGeom g;
  uint32_t lx, ly, lz;
  int grid_scan, grid_pack;  // workgroups of the encode passes (per-device occupancy)
  int ncu;
  uint32_t sample_total;  // 3-D: elements of the codebook sample's bricks inside the field (BrickSample::total)
};

// fills ncu, the encode-pass grids for `device` and sample_total
int brick_configure(BrickLaunch& L, int elem_bytes, int device);

// The codebook sample inside pass 1 (sampled codebook mode): every `stride`-th brick (offset
// stride / 2) is visited FIRST -- iteration j < count takes sample brick j -- and adds its
// histogram to hist (u32[bklen], global atomics); then the word after the bins counts it, and the
// wave that completes the sample publishes it to the host (pub_dst, then *pub_flag = pub_epoch),
// which builds the codebook while pass 1 goes on.  hist == nullptr: no sample, bricks in index order.
// 3-D bricks count relaxed, and the completing wave accepts the sample once its bins sum to total
// (brick_scan.hip finish_brick); linear bricks count with an agent-scope acq_rel and do not use total.
// the sample histogram's bins lie a 64-B line apart: the sample bricks finish together (first
// round of pass 1) and their atomics would otherwise queue on the one or two memory channels of
// a dense 4 KB array (measured: pass 1 +60 us)
constexpr int kSampleBinStride = 16;
struct BrickSample {
  uint32_t* hist = nullptr;  // u32[kMaxBklen * kSampleBinStride + 1]: the bins, then the count of finished sample bricks
  uint32_t stride = 1, count = 0;
  uint32_t total = 0;            // 3-D: elements of the sample bricks inside the field (BrickLaunch::sample_total)
  uint32_t* pub_dst = nullptr;   // host-mapped u32[bklen]
  uint32_t* pub_flag = nullptr;  // host-mapped
  uint32_t pub_epoch = 0;
};
BrickSample brick_sample_plan(const BrickLaunch& L, uint32_t* hist);


// Quant codes between the two encode passes, in brick order (row r of brick b at (64 b + r) W).
// A row whose codes all lie in [c0, c0 + 254] or are 0 (outliers) is stored as bytes (code - c0;
// 255 for code 0) in c8; any other
// row as u16 codes in c16, with bit r of rowmask[b] set.  c0 = radius - 127 (ZigZag: 0): the
// rows that are not u16 are about 90 % of a smooth field's (those off the tiles' first z plane).
struct BrickCodes {
  uint16_t* c16;      // nbricks * 64 * W u16 (written only for the u16 rows)
  uint8_t* c8;        // nbricks * 64 * W bytes
  uint64_t* rowmask;  // nbricks
  uint32_t c0;
};
// pass 1: predict -> global + per-brick histograms, outliers, codes in brick order
template <typename T>
int launch_brick_scan(const BrickLaunch& L, const T* in, double eb, int radius, bool zz, const BrickSample& sample,
                      const OutlierSink& ol,
                      uint32_t* hist, uint16_t* bhist, const BrickCodes& bc, int bklen, hipStream_t st,
                      const HostPub& pub = HostPub{});
// archive plan (brick_pack.hip k_brick_plan): region sizes, cell / outlier offsets, totals, headers
struct BrickPlanArgs {
  const uint16_t* bhist;  // per-brick histograms, stride brick_hist_stride(bklen)
  int bklen, bhs;
  const uint32_t* book;
  uint32_t nbricks, nbx, nby, ly, lz;
  const uint32_t* brick_cnt;  // outliers per brick (pass 1)
  uint32_t cap_per_brick;     // outlier slot capacity per brick
  const uint64_t* slots;      // per-brick outlier slots
  const uint64_t* spill;
  const uint32_t* spill_cnt;
  uint32_t spill_cap;
  uint32_t nblk;              // plan blocks = brick_plan_blocks(nbricks)
  uint32_t* ub;               // per brick: region cells
  uint32_t* cell_local;       // per brick: cell offset inside its plan block
  uint32_t* ol_local;         // per brick: outlier offset inside its plan block
  uint32_t* cell_pre;         // nblk + 1: block prefixes, [nblk] = total cells
  uint32_t* ol_pre;           // nblk + 1: block prefixes, [nblk] = slot outliers
  CompressInfo* info;         // totals
  uint8_t* archive;
  size_t phf_offset, bitstream_rel;
  uint32_t nd = 3;       // 1: 1-D bricks (64 consecutive chunks; the last chunk may be short)
  uint32_t nchunks = 0;  // 1-D: chunks of the field
  size_t n = 0;          // 1-D: elements of the field
  uint32_t* ticket = nullptr;  // 9 words zeroed per call: the two-level last-block ticket
};
uint32_t brick_plan_blocks(uint32_t nbricks);
int brick_hist_stride(int bklen);
int launch_brick_plan(const BrickLaunch& L, const BrickPlanArgs& a, const void* psz_tpl, const void* phf_tpl,
                      hipStream_t st);
// pass 2: brick-ordered codes -> Huffman cells at each brick's reserved region (bricks last to first)
int launch_brick_pack(const BrickLaunch& L, const BrickCodes& bc, const uint32_t* book, int bklen,
                      const BrickPlanArgs& plan, uint32_t* par_nbit, uint32_t* par_entry, uint32_t* bitstream,
                      unsigned int* overflow, hipStream_t st, const HostPub& pub = HostPub{});
struct BrickSingle {
  OutlierSink ol;              // one slot per (brick, y-step): cap_per_brick = the slot's cap
  uint32_t* book;              // device book (the stream kernel's workgroup 0 writes it)
  int bklen;
  uint32_t *par_nbit, *par_entry, *bitstream;
  uint32_t bs_cap;             // bitstream capacity (cells)
  unsigned long long* status;  // nbricks words, zeroed per call
  uint32_t* ticket;            // zeroed per call
  uint32_t* ol_dst;            // per slot: its first cell in the archive's outlier segment
  CompressInfo* info;          // zeroed per call
  unsigned int* timeout;
  uint8_t* archive;
  size_t phf_offset, bits_rel;
  const uint32_t* gate;        // host-mapped: reaches gate_epoch once the host's book is written
  uint32_t gate_epoch;
  const uint32_t* h_book;      // host-mapped book and reverse book
  const uint32_t* h_revbook;
  uint32_t* revbook;           // the archive's reverse book
  int rv_words;
  uint32_t* book_flag;         // device word (never reset)
};
// single-pass mode (brick_stream.hip): the sample histogram into hist (u32[kMaxBklen * kSampleBinStride],
// zeroed; bins one line apart); its last workgroup (ticket: kPubTicketWords words, zeroed) copies
// it to the host-mapped h_hist and sets *flag = epoch; the host builds the codebook.  Then the
// streaming pass, which takes the host's book behind a device-polled gate (+ finish: outlier
// segment, headers, the compress summary)
template <typename T>
int launch_brick_sample(const BrickLaunch& L, const T* in, double eb, int radius, bool zz, uint32_t* hist, int bklen,
                        uint32_t* ticket, uint32_t* h_hist, uint32_t* flag, uint32_t epoch, hipStream_t st);
template <typename T>
int launch_brick_stream(const BrickLaunch& L, const T* in, double eb, int radius, bool zz, const BrickSingle& s,
                        const void* psz_tpl, const void* phf_tpl, hipStream_t st, const HostPub& pub);
// the fused decoders' outlier bounds (BrickOutliers above): k_brick_cell_bounds checks the order
int launch_brick_cell_bounds(const BrickLaunch& L, const uint32_t* cells, size_t ncell, uint32_t* bstart,
                             uint32_t* unsorted, uint32_t epoch, hipStream_t st);
// decode only, any archive whose chunk length is a multiple of 64: chunk c's codes to
// codes[sublen c ...] (index order); called through launch_hf_decode
int launch_chunk_decode(uint32_t ncu, const PhfView& v, uint16_t* codes, size_t n, hipStream_t st);
// fused decode + reconstruct of a 3-D or 1-D brick field (brick3_decode.hip; 1-D: its half in
// brick1_decode.hip, launch_brick1_decode)
template <typename T>
int launch_brick_decode(const BrickLaunch& L, const PhfView& v, T* out, double eb, int radius, bool zz,
                        const BrickOutliers& ol, hipStream_t st);
template <typename T>
int launch_brick1_decode(const BrickLaunch& L, const PhfView& v, T* out, double eb, int radius, bool zz,
                         const BrickOutliers& ol, hipStream_t st);

// Region decode (3-D brick fields, Lorenzo, ranked cells -- the caller has read the bounds pass's
// verdict): the box of e elements at o, decoded from its covering bricks only into out_box, a
// compact array of e (x fastest).  region_box: the covering bricks (lo, n) of a box, brick width W.
struct RegionBox {
  uint32_t ox, oy, oz, ex, ey, ez;        // box, in elements
  uint32_t blx, bly, blz, bnx, bny, bnz;  // covering bricks: first, count
};
RegionBox region_box(uint32_t ox, uint32_t oy, uint32_t oz, uint32_t ex, uint32_t ey, uint32_t ez, uint32_t W);
template <typename T>
int launch_brick_region(const BrickLaunch& L, const PhfView& v, T* out_box, double eb, int radius,
                        const BrickOutliers& ol, const uint32_t (&o)[3], const uint32_t (&e)[3], hipStream_t st);
// Region decode, 1-D brick fields (Lorenzo, chunk length 256, ranked cells, ol.bstart over chunks:
// launch_x1d_bounds with ushift 8): the range of e elements at o, decoded from its covering tiles
// of 1024 only (region_cover.hh region_tiles1) into out_box.
template <typename T>
int launch_brick1_region(const BrickLaunch& L, const PhfView& v, T* out_box, double eb, int radius,
                         const BrickOutliers& ol, size_t o, size_t e, hipStream_t st);
// out_box[(z ey + y) ex + x] = field[((oz + z) ly + oy + y) lx + ox + x] (the region fallback)
template <typename T>
int launch_crop_box(const T* field, size_t lx, size_t ly, const size_t (&o)[3], const size_t (&e)[3], T* out_box,
                    hipStream_t st);

// the outlier cells with lo <= idx < hi into slab[idx - lo] (the region decode's SLAB path); the
// cells in any order
template <typename T>
int launch_scatter_range(const uint32_t* cells, size_t nnz, T* slab, size_t lo, size_t hi, hipStream_t st);

// min / max (Rel mode, extrema.cuhip.inl:86-208), writes {min, max} as doubles
template <typename T>
int launch_extrema(const T* in, size_t n, double* d_minmax, unsigned int* d_scratch, hipStream_t st);

// ---- quality assessment (quality.hip; record and combine: quality_reduce.hh) -----------------
// One pass over reconstruction x and original o, then one small combine launch.  parts: device
// QrPart[kQrGridCap + 1], the workgroups' records and, last, the result.  thr: 1.001 eb, +inf for
// eb == 0.  The grid is qr_grid(len) / qr_region_grid(rows): the combine order depends on nothing else.
struct QrPart;
template <typename T>
int launch_quality(const T* x, const T* o, size_t len, double thr, bool autocor, QrPart* parts, hipStream_t st);
// x: the compact box of e elements; field: the whole original (lx, ly its x and y extents), box at o
template <typename T>
int launch_quality_region(const T* xbox, const T* field, size_t lx, size_t ly, const size_t (&o)[3],
                          const size_t (&e)[3], double thr, bool autocor, QrPart* parts, hipStream_t st);

}  // namespace cusz_amd
