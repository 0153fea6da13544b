// cusz_amd/csrc/pipeline_decode.cc -- the decode side of the Pipeline (pipeline.hh): the codes of
// an archive (Huffman or FZG), the whole field, a box of it (region_plan: which way), spline.
// Every entry clears pend.active: the decoders overwrite the code buffer a pending
// compress_finish would pack, so a scan -> decode -> finish sequence fails cleanly
// (PSZ_AMD_ERR_STATE) instead of writing a corrupt archive.
#include "pipeline.hh"

namespace cusz_amd {

// An archive whose covering slab decodes on its own (the SLAB path): Lorenzo of either kind,
// codes in index order behind Huffman chunks or FZG blocks.
static bool slab_archive(const psz_header* h)
{
  const psz_predictor p = h->pipeline.predictor;
  if (p != Lorenzo && p != LorenzoZigZag) return false;
  if (h->pipeline.codec1 == FZCodec) return h->vle_pardeg > 0;
  return h->pipeline.codec1 == Huffman && h->vle_sublen > 0 && h->vle_pardeg > 0;
}

// A fused candidate of geometry g, for a region decode by k_brick3_decode (3-D) or k_brick1_decode (1-D)
// over the covering bricks: Lorenzo behind Huffman chunks of the brick width (256), one per brick row -- the
// decoder finds a row's chunk by its position.  (An FZG archive has no Huffman chunks to pick bricks by.)
static bool fused_candidate(const psz_header* h, const BrickGeom& g)
{
  return g.ok && g.ndim != 2 && h->pipeline.predictor == Lorenzo && h->pipeline.codec1 == Huffman && h->vle_sublen == g.W &&
         h->vle_pardeg > 0 && (uint32_t)h->vle_pardeg == g.nchunks && 2 * (int)h->rc.radius <= kMaxBklen;
}

// What a region decode of an archive with header h touches (psz_amd_region_plan): the header's
// share of Pipeline::decompress_region's path choice, and the covering bricks.
// mode (PSZ_AMD_REGION_MODE_*): under COVER every Lorenzo archive that is no fused candidate
// takes SLAB, the covering chunks (blocks) of region_cover.hh; WHOLE is the verdict as it was
// before the mode existed.
int region_plan(const psz_header* h, psz_len o, psz_len e, int mode, psz_amd_region_info* out)
{
  if (mode != PSZ_AMD_REGION_MODE_WHOLE && mode != PSZ_AMD_REGION_MODE_COVER) return PSZ_AMD_ERR_INVALID_ARG;
  const psz_len l = h->len;
  if (!box_inside(l, o, e)) return PSZ_AMD_ERR_INVALID_ARG;
  psz_amd_region_info r{};
  r.elems = e.x * e.y * e.z;
  const int nd = ndim_of(l);
  const BrickGeom g = brick_geom(nd, l.x, l.y, l.z, h->dtype == F8 ? 8 : 4);
  const bool fused = fused_candidate(h, g) && (nd == 3 || mode == PSZ_AMD_REGION_MODE_COVER);
  if (fused && nd == 3) {
    const RegionBox b = region_box((uint32_t)o.x, (uint32_t)o.y, (uint32_t)o.z, (uint32_t)e.x, (uint32_t)e.y, (uint32_t)e.z, (uint32_t)g.W);
    r.path = PSZ_AMD_REGION_FUSED;
    r.brick_lo = psz_len{b.blx, b.bly, b.blz};
    r.brick_n = psz_len{b.bnx, b.bny, b.bnz};
    r.bricks = (size_t)b.bnx * b.bny * b.bnz;
    r.chunks = r.bricks * 64;
  }
  else if (fused) {
    // the fused 1-D path (k_brick1_region): the covering tiles of 1024 stand in the brick fields
    const Region1Tiles t = region_tiles1(o.x, e.x);
    r.path = PSZ_AMD_REGION_FUSED;
    r.brick_lo = psz_len{t.t0, 0, 0};
    r.brick_n = psz_len{t.t1 - t.t0, 1, 1};
    r.bricks = t.t1 - t.t0;
    r.chunks = t.chunks(g.nchunks);
  }
  else if (mode == PSZ_AMD_REGION_MODE_COVER && slab_archive(h)) {
    const bool fzg = h->pipeline.codec1 == FZCodec;
    const RegionCover c = region_cover(nd, l.x, l.y, l.z, slow_axis(nd, o), slow_axis(nd, e),
                                       fzg ? (size_t)kFzgBlock : (size_t)h->vle_sublen, (size_t)h->vle_pardeg);
    r.path = PSZ_AMD_REGION_SLAB;
    r.chunks = c.chunks();
  }
  else {
    r.path = PSZ_AMD_REGION_FALLBACK;
    r.chunks = h->vle_pardeg > 0 ? (size_t)h->vle_pardeg : 0;
  }
  *out = r;
  return PSZ_SUCCESS;
}

// An FZG archive before any launch: the psz header's entries on the host, then the segment's own
// 32-byte header and its last offset word, read back in one small synchronous copy (the only
// host wait of an FZG decode).  Everything the decode kernel then loads lies inside the segment;
// flags and offsets inside it that are corrupt are clamped on the device.
int Pipeline::check_fzg(const psz_header* h, const uint8_t* in, FzgHeader* fh)
{
  const psz_predictor pred = h->pipeline.predictor;
  if (pred != Lorenzo && pred != LorenzoZigZag) return PSZ_ABORT_NO_SUCH_CODEC;
  if (h->len.x * h->len.y * h->len.z != n) return PSZ_ABORT_UNSUPPORTED_DIMENSION;
  if (reinterpret_cast<uintptr_t>(in) % 8) return PSZ_AMD_ERR_INVALID_ARG;  // u64 flags and words
  const FzgView v(h, n);
  if (!v.span_ok()) return PSZ_AMD_ERR_BAD_ARCHIVE;
  uint32_t last_off = 0;
  CUSZ_AMD_HIP_CHECK(hipMemcpyAsync(fh, in + v.seg_off, sizeof(FzgHeader), hipMemcpyDeviceToHost, stream));
  CUSZ_AMD_HIP_CHECK(hipMemcpyAsync(&last_off, in + v.seg_off + v.last_off_rel(), 4, hipMemcpyDeviceToHost, stream));
  CUSZ_AMD_HIP_CHECK(hipStreamSynchronize(stream));
  return v.ok(*fh, last_off) ? PSZ_SUCCESS : PSZ_AMD_ERR_BAD_ARCHIVE;
}

int Pipeline::decode_fzg(const psz_header* h, const uint8_t* in, const FzgHeader& fh)
{
  const FzgView v(h, n);
  const uint8_t* seg = in + v.seg_off;
  const FzgDecodeArgs da{reinterpret_cast<const uint64_t*>(seg + v.l.flags_rel), reinterpret_cast<const uint32_t*>(seg + v.l.off_rel),
                         reinterpret_cast<const uint64_t*>(seg + v.l.payload_rel), fh.total_words, n, (int)h->rc.radius,
                         fh.transform, d_codes};
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_fzg_decode(da, stream));
  return PSZ_SUCCESS;
}

int Pipeline::decode_codes(const psz_header* h, const uint8_t* in)
{
  pend.active = false;
  if (h->pipeline.codec1 == FZCodec) {  // (the decoder knob does not apply)
    FzgHeader fh;
    if (const int s = check_fzg(h, in, &fh)) return s;
    return decode_fzg(h, in, fh);
  }
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_hf_decode(PhfView(h, in), n, d_codes, dec_lut(), decoder, ncu, stream));
  return PSZ_SUCCESS;
}

// The bounds pass over the archive's outlier cells (h->splen > 0), and what the reconstructing kernels
// read of it: cells per brick (fused 3-D), per chunk (fused 1-D) or per reconstruction brick (1-D,
// not fused).  Advances the cell epoch; the verdict is the word at ol->unsorted.
int Pipeline::outlier_bounds(const psz_header* h, const uint8_t* in, bool fused, BrickOutliers* ol)
{
  const uint32_t nb = !fused ? geom.nbricks : bl.g.ndim == 1 ? bl.g.nchunks : bl.g.nbricks;
  uint32_t* const flag = d_x1d + nb + 1;
  *ol = BrickOutliers{reinterpret_cast<const uint32_t*>(in + h->entry[PSZHEADER_SPFMT]), (size_t)h->splen, d_x1d, flag, next_cell_epoch()};
  CUSZ_AMD_HIP_CHECK((hipError_t)(
      fused && bl.g.ndim != 1 ? launch_brick_cell_bounds(bl, ol->cells, ol->ncell, d_x1d, flag, ol->epoch, stream)
                              : launch_x1d_bounds(ol->cells, ol->ncell, n, nb, d_x1d, flag, ol->epoch, stream, fused ? 8 : 14)));
  return PSZ_SUCCESS;
}

template <typename T>
int Pipeline::decompress(const psz_header* h, const uint8_t* in, T* out)
{
  pend.active = false;
  const psz_predictor pred = h->pipeline.predictor;
  if (!known_predictor(pred)) return PSZ_ABORT_NO_SUCH_PREDICTOR;
  const bool zz = pred == LorenzoZigZag;
  if (h->len.x != len.x || h->len.y != len.y || h->len.z != len.z) return PSZ_ABORT_UNSUPPORTED_DIMENSION;
  // an FZG archive is checked before anything is written (`out` stays as it is on a bad one)
  const bool fzg = h->pipeline.codec1 == FZCodec;
  FzgHeader fh{};
  if (fzg)
    if (const int s = check_fzg(h, in, &fh)) return s;
  if (pred == Spline) return decompress_spline<T>(h, in, out);
  mark(kMarkDecBegin);
  // fused decode + reconstruct (brick3_decode.hip, brick1_decode.hip): any archive whose chunk length is
  // the brick width, 3-D and 1-D (2-D linear-brick archives decode chunk by chunk); never an FZG archive,
  // whatever its vle_sublen says.  (Wider than fused_candidate: ZigZag too, vle_pardeg not looked at.)
  const bool brickdec = !fzg && bl.g.ok && bl.g.ndim != 2 && decoder == 0 && h->vle_sublen == bl.g.W &&
                        2 * h->rc.radius <= kMaxBklen;
  const uint32_t* cells = reinterpret_cast<const uint32_t*>(in + h->entry[PSZHEADER_SPFMT]);
  // The 1-D reconstruction and the fused brick decoders read sorted cells in place: the fused
  // decoder ranks each row's zero codes against the brick's cells when they are grouped and
  // sorted; only otherwise does the scatter below run (only_if = unsorted).
  BrickOutliers ol;
  if (!zz && h->splen && (brickdec || (geom.ndim == 1 && d_x1d)))
    if (const int s = outlier_bounds(h, in, brickdec, &ol)) return s;
  if (zz) CUSZ_AMD_HIP_CHECK(hipMemsetAsync(out, 0, n * sizeof(T), stream));
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_scatter<T>(cells, h->splen, out, n, stream, ol.unsorted, ol.epoch));
  mark(kMarkScatter);
  if (brickdec) {
    CUSZ_AMD_HIP_CHECK((hipError_t)launch_brick_decode<T>(bl, PhfView(h, in), out, h->rc.eb, h->rc.radius, zz, ol, stream));
    mark(kMarkDecode);
    mark(kMarkRecon);
    return PSZ_SUCCESS;
  }
  int s = fzg ? decode_fzg(h, in, fh) : decode_codes(h, in);
  if (s) return s;
  mark(kMarkDecode);
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_lorenzo_x<T>(d_codes, out, len.x, len.y, len.z, h->rc.eb, h->rc.radius,
                                                     zz, geom, stream, ol.cells ? &ol : nullptr));
  mark(kMarkRecon);
  return PSZ_SUCCESS;
}

// The box of e elements at o into `out` (cusz_amd.h psz_amd_decompress_region_*).  FUSED: only
// the covering bricks are decoded (brick3_decode.hip k_brick3_region), which needs the fused 3-D
// decoder's conditions and ranked outlier cells -- the bounds pass's verdict is the one word
// read back here, before the decode is queued.  FALLBACK: the whole field into a scratch
// field, then the box copied out.  COVER only: FUSED also for 1-D brick archives (k_brick1_region
// over the covering tiles of 1024, the same read-back after launch_x1d_bounds over chunks), and
// SLAB: decompress_slab below.
template <typename T>
int Pipeline::decompress_region(const psz_header* h, const uint8_t* in, psz_len o, psz_len e, T* out)
{
  pend.active = false;
  if (!known_predictor(h->pipeline.predictor)) return PSZ_ABORT_NO_SUCH_PREDICTOR;
  if (h->len.x != len.x || h->len.y != len.y || h->len.z != len.z) return PSZ_ABORT_UNSUPPORTED_DIMENSION;
  psz_amd_region_info info;
  if (const int s = region_plan(h, o, e, region_mode, &info)) return s;
  bool fused = info.path == PSZ_AMD_REGION_FUSED && bl.g.ok && decoder == 0;
  // COVER: a fused candidate that the checks below refuse, and every SLAB verdict, decode the
  // covering slab.  The decoders store 16 bytes at a time from the start of their output, so a
  // chunk length that is no multiple of 8 codes (none this compressor writes) keeps the fallback.
  const bool slab = region_mode == PSZ_AMD_REGION_MODE_COVER && info.path != PSZ_AMD_REGION_FALLBACK &&
                    (h->pipeline.codec1 == FZCodec || h->vle_sublen % 8 == 0);
  BrickOutliers bo;
  if (fused && h->splen) {  // (cells per brick or per chunk, as the full decompress ranks them)
    if (const int s = outlier_bounds(h, in, true, &bo)) return s;
    uint32_t word = 0;
    CUSZ_AMD_HIP_CHECK(hipMemcpyAsync(&word, bo.unsorted, 4, hipMemcpyDeviceToHost, stream));
    CUSZ_AMD_HIP_CHECK(hipStreamSynchronize(stream));
    fused = word != cell_epoch;
  }
  if (fused && ndim == 1)  // (COVER only: region_plan)
    CUSZ_AMD_HIP_CHECK((hipError_t)launch_brick1_region<T>(bl, PhfView(h, in), out, h->rc.eb, h->rc.radius, bo, o.x, e.x, stream));
  else if (fused) {
    // (vle_pardeg == bl.g.nchunks: region_plan)
    const uint32_t o3[3] = {(uint32_t)o.x, (uint32_t)o.y, (uint32_t)o.z}, e3[3] = {(uint32_t)e.x, (uint32_t)e.y, (uint32_t)e.z};
    CUSZ_AMD_HIP_CHECK(
        (hipError_t)launch_brick_region<T>(bl, PhfView(h, in), out, h->rc.eb, h->rc.radius, bo, o3, e3, stream));
  }
  else if (slab) {
    if (const int s = decompress_slab<T>(h, in, o, e, out, &info)) return s;
  }
  else {
    if (!d_region_field) CUSZ_AMD_HIP_CHECK(d_region_field.alloc(n * sizeof(T)));
    if (const int s = decompress<T>(h, in, reinterpret_cast<T*>(d_region_field.p))) return s;
    const size_t o3[3] = {o.x, o.y, o.z}, e3[3] = {e.x, e.y, e.z};
    CUSZ_AMD_HIP_CHECK((hipError_t)launch_crop_box<T>(reinterpret_cast<const T*>(d_region_field.p), len.x, len.y, o3, e3, out, stream));
    const size_t elems = info.elems;
    info = psz_amd_region_info{};
    info.path = PSZ_AMD_REGION_FALLBACK, info.elems = elems;
    info.chunks = h->vle_pardeg > 0 ? (size_t)h->vle_pardeg : 0;
  }
  last_region = info;
  has_last_region = true;
  return PSZ_SUCCESS;
}

// SLAB: the tile-aligned slab [a, b) of the slow axis that covers the box (region_cover.hh), and
// nothing else.  The chunks (blocks) that hold the slab's codes decode to their natural positions
// in d_codes; the outlier cells of the slab go into a slab-sized scratch, in whatever order the
// archive holds them; the slab reconstructs as a field of its own extents (prediction restarts at
// every tile: DESIGN.md §4, "Region decode"), and the box is cropped out of it.  Lorenzo of
// either kind, Huffman in any layout or FZG, any decoder.  No host wait beyond check_fzg's.
template <typename T>
int Pipeline::decompress_slab(const psz_header* h, const uint8_t* in, psz_len o, psz_len e, T* out, psz_amd_region_info* info)
{
  const bool fzg = h->pipeline.codec1 == FZCodec, zz = h->pipeline.predictor == LorenzoZigZag;
  FzgHeader fh{};
  if (fzg) {
    if (const int s = check_fzg(h, in, &fh)) return s;
  }
  const size_t unit = fzg ? (size_t)kFzgBlock : (size_t)h->vle_sublen;
  // (FZG: the segment's own block count, which check_fzg has matched against the field; the full
  // decode does not look at vle_pardeg either)
  const RegionCover c = region_cover(ndim, len.x, len.y, len.z, slow_axis(ndim, o), slow_axis(ndim, e), unit,
                                     fzg ? FzgLayout(n).blocks : (size_t)h->vle_pardeg);
  // 1. codes [c0 unit, min(n, c1 unit)) at their places in d_codes
  const size_t code0 = c.c0 * unit, code1 = std::min(n, c.c1 * unit);
  if (code1 > code0) {
    if (fzg) {
      const FzgView v(h, n);
      const uint8_t* seg = in + v.seg_off;
      const FzgDecodeArgs da{reinterpret_cast<const uint64_t*>(seg + v.l.flags_rel) + (size_t)kFzgBlockUnits * c.c0,
                             reinterpret_cast<const uint32_t*>(seg + v.l.off_rel) + c.c0,
                             reinterpret_cast<const uint64_t*>(seg + v.l.payload_rel), fh.total_words, code1 - code0,
                             (int)h->rc.radius, fh.transform, d_codes + code0};
      CUSZ_AMD_HIP_CHECK((hipError_t)launch_fzg_decode(da, stream));
    }
    else
      CUSZ_AMD_HIP_CHECK((hipError_t)launch_hf_decode(PhfView(h, in).chunks(c.c0, c.c1), code1 - code0, d_codes + code0,
                                                      dec_lut(), decoder, ncu, stream));
  }
  // 2. the slab's scratch: (b - a) P elements
  const size_t lo = c.a * c.P, hi = c.b * c.P, bytes = (hi - lo) * sizeof(T);
  CUSZ_AMD_HIP_CHECK(d_region_slab.grow(bytes));
  T* slab = reinterpret_cast<T*>(d_region_slab.p());
  if (zz) CUSZ_AMD_HIP_CHECK(hipMemsetAsync(slab, 0, bytes, stream));
  // 3. its outlier cells
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_scatter_range<T>(reinterpret_cast<const uint32_t*>(in + h->entry[PSZHEADER_SPFMT]),
                                                         h->splen, slab, lo, hi, stream));
  // 4. reconstruct it as a field of (b - a) steps of the slow axis (the field's own dimension count,
  //    also when one step is left); codes + a P is aligned as the field's rows and planes are
  const size_t sl = c.b - c.a;
  const size_t sx = ndim == 1 ? sl : len.x, sy = ndim == 2 ? sl : len.y, sz = ndim == 3 ? sl : len.z;
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_lorenzo_x<T>(d_codes + lo, slab, sx, sy, sz, h->rc.eb, h->rc.radius, zz,
                                                     lorenzo_geom(ndim, sx, sy, sz, elem_bytes), stream, nullptr));
  // 5. the box out of the slab
  size_t o3[3] = {o.x, o.y, o.z};
  o3[ndim - 1] -= c.a;
  const size_t e3[3] = {e.x, e.y, e.z};
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_crop_box<T>(slab, sx, sy, o3, e3, out, stream));
  const size_t elems = info->elems;
  *info = psz_amd_region_info{};
  info->path = PSZ_AMD_REGION_SLAB, info->elems = elems, info->chunks = c.chunks();
  return PSZ_SUCCESS;
}

// decode -> (outlier buckets) -> spline reconstruct; the archive's outlier cells hold codes
template <typename T>
int Pipeline::decompress_spline(const psz_header* h, const uint8_t* in, T* out)
{
  mark(kMarkDecBegin);
  const size_t words = spline_x_scratch_words(sgeom.ntiles, h->splen);
  if (words > spl_x_words) {
    CUSZ_AMD_HIP_CHECK(d_spl_x.alloc(words));
    spl_x_words = words;
  }
  mark(kMarkScatter);
  int s = decode_codes(h, in);
  if (s) return s;
  mark(kMarkDecode);
  const double eb = h->rc.eb;
  SplineXArgs<T> xa{d_codes, reinterpret_cast<const T*>(in + h->entry[PSZHEADER_ANCHOR]), out,
                    (uint32_t)len.x, (uint32_t)len.y, (uint32_t)len.z, sgeom.gdx, sgeom.gdy, sgeom.gdz, sgeom.ntiles,
                    (float)(1.0 / eb), (float)(eb * 2.0), (int)h->rc.radius};
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_spline3_x<T>(
      xa, reinterpret_cast<const uint32_t*>(in + h->entry[PSZHEADER_SPFMT]), h->splen, d_spl_x, stream));
  mark(kMarkRecon);
  return PSZ_SUCCESS;
}

template int Pipeline::decompress<float>(const psz_header*, const uint8_t*, float*);
template int Pipeline::decompress<double>(const psz_header*, const uint8_t*, double*);
template int Pipeline::decompress_region<float>(const psz_header*, const uint8_t*, psz_len, psz_len, float*);
template int Pipeline::decompress_region<double>(const psz_header*, const uint8_t*, psz_len, psz_len, double*);

}  // namespace cusz_amd
