// cusz_amd/csrc/pipeline.hh -- the compression pipeline behind the cuSZ C API.
//
// Replaces psz::compression_pipeline<T,u2> (psz/src/compressor.inl:268-529) and the C-API
// glue of psz/src/libcusz.cc:219-366.  One device-resident Pipeline per psz_resource:
//
//   compress:  [extrema (Rel)] -> predict+quantize+histogram+outliers (1 kernel)
//              -> histogram D2H, host codebook, book/revbook H2D (the one host round trip
//                 the reference algorithm needs: the codebook depends on the full histogram)
//              -> Huffman encode into the archive (hf_encode.hip: pack, tile sums, gather)
//              -> finalize: outlier compaction + headers written on device
//              -> one 176-B header read-back (compress is synchronous, as in the reference)
//   decompress: outlier scatter -> Huffman decode -> Lorenzo reconstruct (queued, no sync)
//   codec1 = FZCodec (Lorenzo only): predict -> FZG encode (fzg.hip: no codebook stage) -> finalize;
//              decompress: segment check (one 36-B read-back) -> scatter -> FZG decode -> reconstruct
//
// The reference does 5+ host round trips per compress and copies a 2N-byte buffer
// (SURVEY.md §3.1); here the archive is assembled in place.
//
// This header: the buffers, the state and the declarations.  Defined by stage in pipeline.cc (the
// manager), pipeline_compress.cc and pipeline_decode.cc; the C API over it is api_rev1.cc.
//
// What the compress and decode paths share is defined once: the phf segment's offsets and the
// header templates in archive_layout.hh (PhfLayout to write, PhfView to read), the codebook's
// trip through the host and its stream gate in Pipeline::BookGate / book_stage, the small device
// buffer and the host read-back area as the structs SmallBuf / Readback, and every allocation in
// a DevBuf that frees itself.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <tuple>

#include "archive_layout.hh"
#include "common.hh"
#include "cusz_amd.h"
#include "cusz_rev1.h"
#include "kernels.hh"
#include "quality_reduce.hh"
#include "region_cover.hh"

#pragma GCC visibility push(hidden)  // internal to the library: the exports are the C API's
namespace cusz_amd {

inline int ndim_of(psz_len l) { return l.z != 1 ? 3 : l.y != 1 ? 2 : 1; }  // launch.hh:19-28
inline bool known_predictor(psz_predictor p) { return p == Lorenzo || p == LorenzoZigZag || p == Spline; }

// a non-empty box of e elements at o inside a non-empty field of l
inline bool box_inside(psz_len l, psz_len o, psz_len e)
{
  return l.x && l.y && l.z && e.x && e.y && e.z && o.x < l.x && e.x <= l.x - o.x && o.y < l.y && e.y <= l.y - o.y &&
         o.z < l.z && e.z <= l.z - o.z;
}

int region_plan(const psz_header* h, psz_len o, psz_len e, int mode, psz_amd_region_info* out);  // pipeline_decode.cc
void tune_chunking(size_t n, int device, int* sublen, int* pardeg);                    // pipeline.cc

// An allocation that frees itself: device memory, or (Pinned) host memory that is mapped and
// coherent, so that kernels write it and the host polls it.
template <typename T, bool Pinned = false>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { free(); }
  hipError_t alloc(size_t count)  // frees what it holds first
  {
    free();
    if (Pinned) return hipHostMalloc(&p, count * sizeof(T), hipHostMallocMapped | hipHostMallocCoherent);
    return hipMalloc(&p, count * sizeof(T));
  }
  void free() { if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p)), p = nullptr; }
  operator T*() const { return p; }
};

// device bytes that grow on demand and never shrink (what they held is not kept)
struct GrowBuf {
  DevBuf<uint8_t> buf;
  size_t bytes = 0;
  hipError_t grow(size_t need)
  {
    if (need <= bytes) return hipSuccess;
    bytes = 0;
    const hipError_t e = buf.alloc(need);
    if (e == hipSuccess) bytes = need;
    return e;
  }
  uint8_t* p() const { return buf.p; }
};

struct Event {  // likewise
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { if (e) (void)hipEventDestroy(e); }
  operator hipEvent_t() const { return e; }
};

// The small device buffer (Pipeline::d_small).  Bytes [0, kSmallZeroBytes) are zeroed at the start
// of every compress; the tickets are the 9-word publish tickets of pub_device.hh.
struct SmallBuf {
  uint32_t spill_cnt, pad0[3];
  unsigned int timeout, code_lost, hist_missing, pad1[9];  // code_lost: spline codes no outlier cell can carry;
                                                           // hist_missing: a caller's histogram lacks a used bin
  CompressInfo info;
  uint32_t plan_ticket[9], pad2[3];
  uint32_t hist_ticket[9];
  uint32_t summary_ticket[9];
  uint32_t pad3[2];
  uint32_t book_flag, pad4[3];  // the single-pass mode's codebook flag (brick_stream.hip k_brick3_stream):
                                // never zeroed, epoch-compared
  double minmax[2];
  uint8_t pad5[240];
  unsigned int ext_scratch[2 * 1024 * 2];  // extrema scratch
  uint32_t dec_lut[kHfDecScratchWords];
};
constexpr size_t kSmallBytes = sizeof(SmallBuf);
constexpr size_t kSmallZeroBytes = offsetof(SmallBuf, summary_ticket) + sizeof(SmallBuf::summary_ticket);
static_assert(offsetof(SmallBuf, spill_cnt) == 0 && offsetof(SmallBuf, timeout) == 16 && offsetof(SmallBuf, code_lost) == 20 &&
                  offsetof(SmallBuf, hist_missing) == 24 && offsetof(SmallBuf, info) == 64 &&
                  offsetof(SmallBuf, plan_ticket) == 112 && offsetof(SmallBuf, hist_ticket) == 160 &&
                  offsetof(SmallBuf, summary_ticket) == 196 && offsetof(SmallBuf, book_flag) == 240 &&
                  offsetof(SmallBuf, minmax) == 256 && offsetof(SmallBuf, ext_scratch) == 512 &&
                  offsetof(SmallBuf, dec_lut) == 512 + 2 * 1024 * 8 && kSmallZeroBytes == 232 &&
                  kSmallBytes == 512 + 2 * 1024 * 8 + kHfDecScratchWords * 4,
              "small-buffer layout");

// The 1 KB read-back area of the host-mapped transfer buffer (Pipeline::h_readback): what the
// publish kernels copy to the host.
struct Readback {
  uint8_t header[sizeof(psz_header)], pad0[80];  // the archive's psz header
  CompressInfo info;
  uint8_t pad1[80];
  unsigned int timeout, code_lost, hist_missing, pad2[13];  // read back together (SmallBuf keeps them adjacent;
                                                            // hist_missing with a caller's histogram only)
  uint32_t excess, pad3[15];  // a sharded finish's summed overflow word
  double minmax[2];           // Rel mode's extrema
};
static_assert(offsetof(Readback, header) == 0 && offsetof(Readback, info) == 256 && offsetof(Readback, timeout) == 384 &&
                  offsetof(Readback, code_lost) == 388 && offsetof(Readback, hist_missing) == 392 &&
                  offsetof(Readback, excess) == 448 && offsetof(Readback, minmax) == 512 && sizeof(Readback) <= 1024,
              "read-back layout");

// The words of the host-mapped transfer area that device and host signal each other through
// (Pipeline::flag): each carries the epoch of the hand-over it last completed.
enum HostFlag {
  kFlagRange = 1,    // Rel mode's extrema are in the read-back area
  kFlagHist = 2,     // the histogram (or the codebook sample) is in h_hist()
  kFlagSummary = 3,  // header + summary of a compress are in the read-back area
  kFlagGate = 5,     // host -> device: the codebook is in h_book() / h_revbook()
};

// Timing events (Pipeline::mark): the start of a compress, then the end of each of its stages
// (PSZ_AMD_T_*); likewise for a decompress.
enum Mark {
  kMarkBegin, kMarkExtrema, kMarkPredict, kMarkBook, kMarkEncode, kMarkFinalize,
  kMarkDecBegin, kMarkScatter, kMarkDecode, kMarkRecon,
  kMarkCount
};

// How a compress goes on after the predictor (Pipeline::choose_path).
enum class Path {
  Reference,  // Lorenzo, codes in index order -> Huffman in the reference layout
  Spline,     // spline3 -> the same
  Fzg,        // Lorenzo -> FZG encode (codec1 = FZCodec: no codebook)
  Brick,      // fused bricks: pass 1, plan, pass 2 straight into the archive
  Stream      // fused bricks, single pass behind a sampled book (PSZ_AMD_CODEBOOK_STREAM)
};

struct Pipeline {
  psz_dtype dtype;
  psz_len len;
  size_t n = 0;
  int ndim = 1;
  int device = 0;
  int ncu = 0;  // the device's compute units (init)
  hipStream_t stream = nullptr;
  int elem_bytes = 4;

  LorenzoGeom geom{};
  BrickLaunch bl{};               // fused brick path (brick_*.hip); bl.g.ok when eligible
  int layout = 0;                 // PSZ_AMD_LAYOUT_*: 0 brick layout when eligible, 1 reference layout
  bool layout_set = false;        // PSZ_AMD_LAYOUT_BRICK_FORCE: bricks also for small 2-D fields
  int codebook = PSZ_AMD_CODEBOOK_SAMPLED;  // PSZ_AMD_CODEBOOK_*: sampled device book (default),
                                            // reference book (exact), streaming single pass
  DevBuf<uint32_t> d_shist;       // pass 1's codebook sample: strided histogram + counter
  DevBuf<uint16_t> d_bhist;       // per-brick u16 histograms (pass 1 -> reservation)
  DevBuf<uint32_t> d_ub;          // per-brick region upper bounds (cells)
  DevBuf<uint32_t> d_bbase;       // per-brick cell offsets inside their plan block
  DevBuf<uint32_t> d_plan;        // plan block prefixes: cells | outliers (nblk + 1 each)
  SplineGeom sgeom{};
  uint32_t spl_cap = 0;           // outlier slots per spline tile
  DevBuf<uint64_t> d_spl_slots;   // ntiles * spl_cap cells (allocated on first use)
  DevBuf<uint32_t> d_spl_cnt;     // per-tile outlier counts | offsets
  DevBuf<uint32_t> d_spl_off;
  DevBuf<uint32_t> d_spl_sps;     // per-tile spill range starts
  DevBuf<uint32_t> d_spl_x;       // decompression buckets
  DevBuf<uint32_t> d_x1d;         // decompression: per-unit first outlier cell + unsorted flag (1-D; fused bricks)
  uint32_t cell_epoch = 0;        // tags the unsorted flag of the current decompress (never 0)
  uint32_t next_cell_epoch() { return cell_epoch = cell_epoch + 1 ? cell_epoch + 1 : 1; }
  DevBuf<uint8_t> d_region_field;  // region fallback: the whole field (allocated on first use)
  GrowBuf d_region_slab;           // region SLAB path: the covering slab.  It only grows: the largest slab a
                                   // manager has decoded stays allocated until the manager is released
  int region_mode = PSZ_AMD_REGION_MODE_WHOLE;  // PSZ_AMD_REGION_MODE_*
  DevBuf<QrPart> d_quality;        // quality assessment: workgroup records + the result (allocated on first use)
  psz_amd_region_info last_region{};
  bool has_last_region = false;
  size_t spl_x_words = 0;
  int sublen = 256, pardeg = 1;
  int user_sublen = 0;
  int tuned_sublen = 256;  // tune_chunking's choice for this field
  int decoder = 0;  // PSZ_AMD_DECODER_*
  uint32_t cap_per_brick = 0, spill_cap = 0;
  size_t splen = 0;

  // device
  DevBuf<uint16_t> d_codes;
  DevBuf<uint8_t> d_codes8;        // brick layout: byte rows between the encode passes
  DevBuf<uint64_t> d_rowmask;      // brick layout: u16 rows per brick
  DevBuf<uint32_t> d_hist;
  DevBuf<uint32_t> d_book;
  DevBuf<uint64_t> d_slots;
  DevBuf<uint32_t> d_brick_cnt;
  DevBuf<uint32_t> d_brick_off;
  DevBuf<uint64_t> d_spill;
  DevBuf<SmallBuf> d_small;  // one SmallBuf
  DevBuf<uint32_t> d_enc_temp;     // encoder scratch (chunk cells at a worst-case stride)
  DevBuf<uint8_t> d_archive;
  size_t archive_cap = 0;

  // pinned, host-mapped, coherent transfer area (kernels write it, the host polls flags)
  DevBuf<uint8_t, true> h_xfer;
  uint32_t epoch = 0;
  uint32_t gate_epoch = 0;       // host -> stream gate (kFlagGate): the upload kernel polls it
  uint32_t summary_epoch = 0;    // the epoch with which a finish's last kernel publishes the summary (summary_pub)
  bool gate = true;              // brick encode queued behind a device-polled host gate (kFlagGate)
  static constexpr size_t kXferBytes = 16384;
  // 16 flag words; every host access is an __atomic_load_n / __atomic_store_n
  uint32_t* flag(HostFlag f) { return reinterpret_cast<uint32_t*>(h_xfer.p) + f; }
  uint32_t* h_hist() { return reinterpret_cast<uint32_t*>(h_xfer.p + 64); }               // 4 KB
  uint32_t* h_book() { return reinterpret_cast<uint32_t*>(h_xfer.p + 64 + 4096); }        // 4 KB
  uint8_t* h_revbook() { return h_xfer.p + 64 + 8192; }                                    // 2304 B
  Readback* h_readback() const { return reinterpret_cast<Readback*>(h_xfer.p + 64 + 8192 + 2560); }  // 1 KB

  bool timing = false;
  bool broken = false;  // an allocation failed mid-call (regrow): every later compress fails
  Event ev[kMarkCount];
  float stage_ms[PSZ_AMD_T_COUNT] = {0};

  uint32_t* spill_cnt() { return &d_small.p->spill_cnt; }
  unsigned int* timeout() { return &d_small.p->timeout; }
  unsigned int* hist_missing() { return &d_small.p->hist_missing; }
  CompressInfo* info() { return &d_small.p->info; }
  double* minmax() { return d_small.p->minmax; }
  unsigned int* ext_scratch() { return d_small.p->ext_scratch; }
  uint32_t* dec_lut() { return d_small.p->dec_lut; }
  uint32_t* hist_ticket() { return d_small.p->hist_ticket; }
  uint32_t* summary_ticket() { return d_small.p->summary_ticket; }
  uint32_t* plan_ticket() { return d_small.p->plan_ticket; }
  uint32_t* book_flag() { return &d_small.p->book_flag; }
  static constexpr uint32_t kStreamSlots = 8;  // outlier slots per brick in the single-pass mode (one per y-step)

  // outlier slot per brick of the brick layout: 10 % of its elements + 16 at first; a compress
  // whose bricks spill grows it to the largest brick's count (grow_slots)
  uint32_t brick_slot_cap = 0;
  // cells of every slot (the bricks of the reference layout and of the brick layout share d_slots)
  size_t slot_cells_total() const
  {
    size_t c = (size_t)geom.nbricks * cap_per_brick;
    if (bl.g.ok) c = std::max(c, (size_t)bl.g.nbricks * brick_slot_cap);
    return c;
  }
  int grow_events = 0;  // capacity growths (a compress that warned repeats only after one)
  size_t bitstream_cells_cap() const { return (n * kLmax + 31) / 32 + (size_t)pardeg + 8; }

  // state carried from compress_scan (pass 1) to compress_finish (codebook onwards)
  struct Pending {
    bool active = false;
    Path path = Path::Reference;  // of the last scan that got past its checks
    bool zz = false;
    int radius = 0;
    uint32_t hist_epoch = 0;  // != 0: the scan published d_hist to h_hist() with this epoch (kFlagHist)
    bool ext = false;         // finish with a caller's (reduced) histogram + overflow word
    bool side_book = false;   // pass 1 publishes a codebook sample to the host (epoch: hist_epoch)
    size_t anchor_bytes = 0;
  } pend;
  bool bricks() const { return pend.path == Path::Brick || pend.path == Path::Stream; }
  // layout of the last compress (PSZ_AMD_LAYOUT_*)
  int last_layout() const { return bricks() ? PSZ_AMD_LAYOUT_BRICK : PSZ_AMD_LAYOUT_REFERENCE; }

  // ---- pipeline.cc: the manager ----
  int init(psz_dtype dt, psz_len l, void* st);
  hipError_t alloc_chunk_state();
  template <typename T>
  int regrow(DevBuf<T>& buf, size_t count);
  int regrown();
  int grow_spill(uint64_t need);
  int grow_slots(uint32_t need);
  int fetch(XferRegions r, HostFlag fl);
  int wait_flag(HostFlag fl, uint32_t e);
  static XferRegions regions(std::initializer_list<std::tuple<void*, const void*, size_t>> l);
  void mark(Mark i) { if (timing) (void)hipEventRecord(ev[i], stream); }
  float span(Mark a, Mark b);
  void collect_decompress_times();

  // ---- pipeline_compress.cc ----
  struct Choice { int status; Path path; bool zz; int radius, bklen; };  // status != PSZ_SUCCESS: refused
  Choice choose_path(const psz_header* h, bool single) const;
  template <typename T>
  int scale_rel_eb(psz_header* h, const T* in);
  // The codebook's trip through the host: the histogram arrives with epoch eh (kFlagHist), the host
  // builds the book, and -- when armed -- opens the gate (kFlagGate = eg) that the launches queued
  // behind the book poll on the device.  A local object of each finish: a stream waiting on
  // a gate that never opens hangs every later call on it, so the destructor opens an armed gate
  // on every path out, the early error returns included.
  struct BookGate {
    Pipeline& p;
    int bklen;
    uint32_t eh = 0, eg = 0;
    bool armed = false;
    ~BookGate() { open(); }
    void open() { if (armed) __atomic_store_n(p.flag(kFlagGate), eg, __ATOMIC_RELEASE), armed = false; }
    int build(bool twoqueue);
    int build_if_armed(bool twoqueue) { return armed ? build(twoqueue) : PSZ_SUCCESS; }  // (else: built already, or no host book)
  };
  int book_stage(BookGate& g, bool twoqueue, const PhfLayout& lay);
  struct PhfSections { uint32_t *par_nbit, *par_entry, *bits; };
  PhfSections phf_sections(const PhfLayout& lay) const;
  HostPub hist_pub(int bklen);
  HostPub summary_pub();
  XferRegions hist_regions(int bklen);
  XferRegions readback_regions();
  BrickCodes brick_codes(bool zz, int radius) const;
  template <typename T>
  int compress(psz_header* h, const T* in, uint8_t** out, size_t* outlen);
  template <typename T>
  int compress_scan(psz_header* h, const T* in, bool single = false);
  int compress_finish(psz_header* h, const uint32_t* ext_hist, uint8_t** out, size_t* outlen, const void* in = nullptr);
  int finish_huffman(psz_header* h, uint8_t** out, size_t* outlen);
  int finish_fzg(psz_header* h, uint8_t** out, size_t* outlen);
  int finish_brick(psz_header* h, uint8_t** out, size_t* outlen);
  template <typename T>
  int finish_stream(psz_header* h, const T* in, uint8_t** out, size_t* outlen);
  int finalize_outliers(const psz_header* h, const void* seg_tpl, size_t seg_off, size_t data_rel, const uint32_t* par_nbit,
                        const uint32_t* par_entry, int npar);
  int finish_compress(psz_header* h, uint8_t** out, size_t* outlen);

  // ---- pipeline_decode.cc ----
  int check_fzg(const psz_header* h, const uint8_t* in, FzgHeader* fh);
  int decode_fzg(const psz_header* h, const uint8_t* in, const FzgHeader& fh);
  int decode_codes(const psz_header* h, const uint8_t* in);
  int outlier_bounds(const psz_header* h, const uint8_t* in, bool fused, BrickOutliers* ol);
  template <typename T>
  int decompress(const psz_header* h, const uint8_t* in, T* out);
  template <typename T>
  int decompress_region(const psz_header* h, const uint8_t* in, psz_len o, psz_len e, T* out);
  template <typename T>
  int decompress_slab(const psz_header* h, const uint8_t* in, psz_len o, psz_len e, T* out, psz_amd_region_info* info);
  template <typename T>
  int decompress_spline(const psz_header* h, const uint8_t* in, T* out);
};

}  // namespace cusz_amd
#pragma GCC visibility pop
