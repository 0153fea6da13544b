// cusz_amd/csrc/pipeline.cc -- the Pipeline (pipeline.hh) as a manager: creation, the buffers
// sized by the chunking and their growth, the small transfers through host-mapped memory, timing.
#include "pipeline.hh"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace cusz_amd {

int report_hip_error(hipError_t e, const char* expr, const char* file, int line)
{
  std::fprintf(stderr, "[cusz_amd] HIP error %d (%s) at %s:%d: %s\n", (int)e, hipGetErrorString(e), file, line,
               expr);
  return PSZ_AMD_ERR_DEVICE;
}

// Chunk length (vle_sublen).  The reference sizes chunks for one encode thread per chunk on
// maxThreadsPerBlock * nSM / 4 threads (libphf.cc:26-70, which notes "ROCm GPUs should use
// different constants").  Here the decoder is the consumer that needs the parallelism: one lane
// per chunk, two waves per SIMD -> nCU * 4 SIMDs * 64 lanes * 2 chunks (131,072 on MI355X, so
// 512^3 gets sublen 1024, the reference's own HFR setting, hf_buf.cc:77).  Multiple of 256,
// at most 8192 (encoder LDS); any value is readable by either decoder.
void tune_chunking(size_t n, int device, int* sublen, int* pardeg)
{
  int ncu = 256;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu < 1) ncu = 256;
  const size_t lanes = (size_t)ncu * 4 * 64 * 2;
  size_t s = (std::max<size_t>(n, 1) - 1) / lanes + 1;
  s = ((s - 1) / 256 + 1) * 256;
  if (s > 8192) s = 8192;
  *sublen = (int)s;
  *pardeg = (int)((std::max<size_t>(n, 1) - 1) / s + 1);
}

int Pipeline::init(psz_dtype dt, psz_len l, void* st)
{
  dtype = dt;
  len = l;
  if (l.x == 0 || l.y == 0 || l.z == 0) return PSZ_ABORT_UNSUPPORTED_DIMENSION;
  n = l.x * l.y * l.z;
  if (n >= (1ull << 32)) return PSZ_ABORT_UNSUPPORTED_DIMENSION;  // u32 outlier index (sp_interface.h)
  ndim = ndim_of(l);
  elem_bytes = dt == F8 ? 8 : 4;
  // the 2-D Lorenzo kernels address one row through a 32-bit buffer range: a row of 2 GiB or
  // more is a shape this build does not take (creation fails with this status; the caller
  // reshapes such a field to 1-D)
  if (ndim == 2 && l.x * (size_t)elem_bytes >= 0x80000000ull) return PSZ_ABORT_UNSUPPORTED_DIMENSION;
  stream = (hipStream_t)st;
  CUSZ_AMD_HIP_CHECK(hipGetDevice(&device));
  CUSZ_AMD_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
  tune_chunking(n, device, &sublen, &pardeg);
  tuned_sublen = sublen;
  geom = lorenzo_geom(ndim, l.x, l.y, l.z, elem_bytes);
  sgeom = spline_geom(l.x, l.y, l.z);
  spl_cap = (uint32_t)(std::min<size_t>(l.x, 32) * std::min<size_t>(l.y, 8) * std::min<size_t>(l.z, 8) / 10 + 16);
  // outlier capacity: 10 % of the input like the reference (buf_comp.hh:55), as per-brick
  // slots plus an equally large spill list for bricks above 10 %.
  cap_per_brick = geom.brick_elems / 10 + 16;
  spill_cap = (uint32_t)(n / 10 + 1024);
  bl.g = brick_geom(ndim, l.x, l.y, l.z, elem_bytes);
  bl.lx = (uint32_t)l.x, bl.ly = (uint32_t)l.y, bl.lz = (uint32_t)l.z;
  uint32_t max_bricks = geom.nbricks;
  if (bl.g.ok) {
    CUSZ_AMD_HIP_CHECK((hipError_t)brick_configure(bl, elem_bytes, device));
    brick_slot_cap = bl.g.brick_elems / 10 + 16;
    max_bricks = std::max(max_bricks, bl.g.nbricks);
    CUSZ_AMD_HIP_CHECK(d_bhist.alloc((size_t)bl.g.nbricks * kMaxBklen));
    CUSZ_AMD_HIP_CHECK(d_ub.alloc(bl.g.nbricks));
    CUSZ_AMD_HIP_CHECK(d_bbase.alloc((size_t)bl.g.nbricks + 1));
    CUSZ_AMD_HIP_CHECK(d_plan.alloc(2 * ((size_t)brick_plan_blocks(bl.g.nbricks) + 1)));
    CUSZ_AMD_HIP_CHECK(d_codes8.alloc((size_t)bl.g.nbricks * bl.g.brick_elems + 64));  // + 8-B load slack
    CUSZ_AMD_HIP_CHECK(d_rowmask.alloc(bl.g.nbricks));
  }
  // decompression's per-unit first outlier cell + unsorted word.  1-D: units of 16384 elements
  // (reconstruction) or 256 (brick chunks); the fused decoders: one unit per brick
  const size_t x1d_units = std::max<size_t>(ndim == 1 ? std::max<size_t>(geom.nbricks, (n + 255) / 256) : 0, bl.g.ok ? bl.g.nbricks : 0);
  if (x1d_units) {
    CUSZ_AMD_HIP_CHECK(d_x1d.alloc(x1d_units + 2));
    CUSZ_AMD_HIP_CHECK(hipMemset(d_x1d, 0, (x1d_units + 2) * 4));  // unsorted word: no epoch yet
  }

  // codes: index order (reference layout) or brick order (brick layout: whole bricks)
  const size_t code_len = std::max(n + 64, bl.g.ok ? (size_t)bl.g.nbricks * bl.g.brick_elems : 0);
  CUSZ_AMD_HIP_CHECK(d_codes.alloc(code_len));
  CUSZ_AMD_HIP_CHECK(d_hist.alloc(kMaxBklen + 4));  // + the sharded overflow word
  CUSZ_AMD_HIP_CHECK(d_book.alloc(kMaxBklen));
  CUSZ_AMD_HIP_CHECK(d_slots.alloc(slot_cells_total()));
  CUSZ_AMD_HIP_CHECK(d_brick_cnt.alloc(max_bricks));
  CUSZ_AMD_HIP_CHECK(d_brick_off.alloc((size_t)max_bricks + 1));
  CUSZ_AMD_HIP_CHECK(d_spill.alloc(spill_cap));
  CUSZ_AMD_HIP_CHECK(d_small.alloc(1));
  CUSZ_AMD_HIP_CHECK(hipMemset(d_small, 0, kSmallBytes));
  CUSZ_AMD_HIP_CHECK(alloc_chunk_state());
  CUSZ_AMD_HIP_CHECK(h_xfer.alloc(kXferBytes));
  std::memset(h_xfer, 0, kXferBytes);
  for (auto& e : ev) CUSZ_AMD_HIP_CHECK(hipEventCreate(&e.e));
  if (bl.g.ok)  // pass 1's sample: strided histogram + the done counter
    CUSZ_AMD_HIP_CHECK(d_shist.alloc((size_t)kMaxBklen * kSampleBinStride + 16));
  if (const char* g = getenv("CUSZ_AMD_NO_GATE")) gate = atoi(g) == 0;
  return PSZ_SUCCESS;
}

// What the chunking sizes: the encoder's scratch and the archive (its worst case).
hipError_t Pipeline::alloc_chunk_state()
{
  d_enc_temp.free();
  if (const size_t tw = hf_encode_temp_words(sublen, pardeg)) {
    const hipError_t et = d_enc_temp.alloc(tw);
    if (et != hipSuccess) return et;
  }
  d_archive.free();
  const size_t ol_cells = std::max(slot_cells_total(), (size_t)sgeom.ntiles * spl_cap);
  // chunk tables: the tuned chunking's, or the brick layout's (one chunk per brick row)
  const size_t chunks = std::max((size_t)pardeg, bl.g.ok ? (size_t)bl.g.nchunks : 0);
  const PhfLayout lay((size_t)elem_bytes * sgeom.anchor_len, kMaxBklen, chunks);
  archive_cap = lay.phf_off + lay.bits_rel + 4 * (bitstream_cells_cap() + chunks) + 8 * (ol_cells + spill_cap) + 64;
  // an FZG archive's worst case (every bit-plane word nonzero: 2 n bytes of payload + flags +
  // offsets) lies below the Huffman bound of 27 bits a symbol; sized explicitly all the same
  const FzgLayout fz(n);
  archive_cap = std::max(archive_cap, fz.fzg_off + fz.worst_bytes() + 8 * (ol_cells + spill_cap) + 64);
  return d_archive.alloc(archive_cap);
}

// buf <- a new allocation of `count`; the old one is freed only once the new one exists.  On
// failure the manager is marked broken (every later compress returns PSZ_AMD_ERR_DEVICE instead
// of handing a kernel a null list or archive) and -1 returned.
template <typename T>
int Pipeline::regrow(DevBuf<T>& buf, size_t count)
{
  DevBuf<T> grown;
  if (grown.alloc(count) != hipSuccess) return broken = true, -1;
  std::swap(buf.p, grown.p);  // (grown frees the old allocation)
  return 0;
}

// after a regrow: the archive to match.  1: grown, -1: allocation failure (manager marked broken)
int Pipeline::regrown()
{
  if (alloc_chunk_state() != hipSuccess) return broken = true, -1;
  grow_events++;
  return 1;
}

// Outlier capacity beyond the reference's 10 % (buf_comp.cc:87-88, compressor.inl:368-372 fail
// the compress there): a spill list for `need` cells (bounded by n) and an archive to match.
// 1: grown, 0: already at the bound, -1: allocation failure.
int Pipeline::grow_spill(uint64_t need)
{
  const uint64_t cap = std::min<uint64_t>(need + need / 8 + 1024, (uint64_t)n + 1024);
  if (cap <= spill_cap) return 0;
  if (regrow(d_spill, cap)) return -1;
  spill_cap = (uint32_t)cap;
  return regrown();
}

// Bricks with more outliers than their slot spilled to the shared list (archive valid, but the
// list's order depends on the atomics, so the archive is not deterministic and the decoders
// take the scatter path).  The slots of the layout just used grow to the largest brick's count
// (bounded by the brick's elements) and the caller repeats: identical below the 10 % slots.
// 1: grown, 0: already at the bound, -1: allocation failure (manager marked broken).
int Pipeline::grow_slots(uint32_t need)
{
  uint32_t& cap = bricks() ? brick_slot_cap : cap_per_brick;
  const uint32_t lim = bricks() ? bl.g.brick_elems : geom.brick_elems;
  const uint32_t want = (uint32_t)std::min<uint64_t>(lim, (uint64_t)need + need / 8 + 16);
  if (want <= cap) return 0;
  cap = want;
  if (regrow(d_slots, slot_cells_total())) return -1;
  return regrown();
}

// device words -> host-mapped memory, then wait for the flag (fallback: stream sync)
int Pipeline::fetch(XferRegions r, HostFlag fl)
{
  const uint32_t e = ++epoch;
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_publish(r, flag(fl), e, stream));
  return wait_flag(fl, e);
}

int Pipeline::wait_flag(HostFlag fl, uint32_t e)
{
  for (long spin = 0;; spin++) {
    if (__atomic_load_n(flag(fl), __ATOMIC_ACQUIRE) == e) return PSZ_SUCCESS;
    if (spin > (1L << 26)) break;  // ~seconds: something is wrong, surface it via the runtime
    __builtin_ia32_pause();
  }
  CUSZ_AMD_HIP_CHECK(hipStreamSynchronize(stream));
  return __atomic_load_n(flag(fl), __ATOMIC_ACQUIRE) == e ? PSZ_SUCCESS : PSZ_AMD_ERR_DEVICE;
}

XferRegions Pipeline::regions(std::initializer_list<std::tuple<void*, const void*, size_t>> l)
{
  XferRegions r{};
  for (auto& [d, s, bytes] : l) {
    r.dst[r.count] = (uint32_t*)d;
    r.src[r.count] = (const uint32_t*)s;
    r.nwords[r.count] = (int)((bytes + 3) / 4);
    r.count++;
  }
  return r;
}

float Pipeline::span(Mark a, Mark b)
{
  float ms = 0;
  if (hipEventElapsedTime(&ms, ev[a], ev[b]) != hipSuccess) ms = -1;
  return ms;
}

void Pipeline::collect_decompress_times()
{
  if (!timing) return;
  (void)hipEventSynchronize(ev[kMarkRecon]);
  stage_ms[PSZ_AMD_T_SCATTER] = span(kMarkDecBegin, kMarkScatter);
  stage_ms[PSZ_AMD_T_DECODE] = span(kMarkScatter, kMarkDecode);
  stage_ms[PSZ_AMD_T_RECON] = span(kMarkDecode, kMarkRecon);
  stage_ms[PSZ_AMD_T_DECOMPRESS] = span(kMarkDecBegin, kMarkRecon);
}

}  // namespace cusz_amd
