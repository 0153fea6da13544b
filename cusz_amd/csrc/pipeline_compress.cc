// cusz_amd/csrc/pipeline_compress.cc -- the compress side of the Pipeline (pipeline.hh).
//
// choose_path decides once how a compress runs; compress_scan is pass 1 (extrema, predictor,
// histogram, outliers), compress_finish the rest by path: codebook (book_stage behind a BookGate),
// encode into the archive, finalize.  finish_compress reads the summary back and reports.
#include <cstdio>
#include <cstring>

#include "codebook.hh"
#include "pipeline.hh"

namespace cusz_amd {

// The one decision of how a compress runs, and the one validation of predictor, codec1 and radius
// (in this order, before any launch).  single: the single-process compress(), which alone may take
// the streaming single pass; a scan (sharded callers) never does.
Pipeline::Choice Pipeline::choose_path(const psz_header* h, bool single) const
{
  const psz_predictor pred = h->pipeline.predictor;
  const bool fzg = h->pipeline.codec1 == FZCodec;
  Choice c{PSZ_SUCCESS, Path::Reference, pred == LorenzoZigZag, h->rc.radius, 2 * h->rc.radius};
  if (!known_predictor(pred)) return c.status = PSZ_ABORT_NO_SUCH_PREDICTOR, c;
  if ((h->pipeline.codec1 != Huffman && !fzg) || (fzg && pred == Spline)) return c.status = PSZ_ABORT_NO_SUCH_CODEC, c;
  if (c.radius < 1 || c.bklen > kMaxBklen) return c.status = PSZ_AMD_ERR_INVALID_ARG, c;
  // fused bricks: an eligible shape, Lorenzo, default chunking (chunk = brick row).  2-D linear
  // bricks by default only when there are enough to fill the device (a wave walks a brick
  // serially: 3600 x 1800 has 396, the reference layout is faster there)
  const bool enough = bl.g.ndim != 2 || layout_set || bl.g.nbricks >= 4u * (uint32_t)bl.ncu;
  const bool brick = bl.g.ok && layout == 0 && enough && (user_sublen == 0 || user_sublen == bl.g.W);
  if (pred == Spline)
    c.path = Path::Spline;
  else if (fzg)  // Lorenzo's codes in index order, whatever the layout and codebook knobs say
    c.path = Path::Fzg;
  else if (brick)
    c.path = single && codebook == PSZ_AMD_CODEBOOK_STREAM && bl.g.ndim == 3 ? Path::Stream : Path::Brick;
  return c;
}

// Rel mode: eb *= (max - min)  (libcusz.cc:287-293; range in double of T extrema)
template <typename T>
int Pipeline::scale_rel_eb(psz_header* h, const T* in)
{
  if (h->rc.mode != Rel) return PSZ_SUCCESS;
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_extrema<T>(in, n, minmax(), ext_scratch(), stream));
  if (int fs = fetch(regions({{h_readback()->minmax, minmax(), 16}}), kFlagRange)) return fs;
  double mm[2];
  std::memcpy(mm, h_readback()->minmax, 16);
  h->min_val = mm[0], h->max_val = mm[1];
  h->rc.eb *= (mm[1] - mm[0]);
  return PSZ_SUCCESS;
}

// twoqueue: the two-queue book of histogram + 1 (a sample: every code encodable; codebook.cc),
// else the reference's heap on the full histogram
int Pipeline::BookGate::build(bool twoqueue)
{
  const int fs = p.wait_flag(kFlagHist, eh);
  if (!fs) {
    if (twoqueue)
      build_codebook_twoqueue(p.h_hist(), bklen, 1u, p.h_book(), p.h_revbook());
    else
      build_codebook(p.h_hist(), bklen, p.h_book(), p.h_revbook());
  }
  open();  // always open the gate
  return fs;
}

// The codebook stage of finish_huffman and finish_brick: book and reverse book (the latter
// into the archive) from the device histogram.  Host book: the histogram is published now unless
// pass 1 did, and the book is uploaded behind the gate, which g.build() opens once the caller
// has queued its remaining launches (g.armed) -- or, ungated (CUSZ_AMD_NO_GATE), built here and
// uploaded plainly.  Otherwise (spline, a sharded finish) the device book, no host round trip.
int Pipeline::book_stage(BookGate& g, bool twoqueue, const PhfLayout& lay)
{
  uint8_t* revbook = d_archive + lay.phf_off + lay.rvbk_rel;
  if (codebook != PSZ_AMD_CODEBOOK_EXACT && pend.hist_epoch == 0) {
    CUSZ_AMD_HIP_CHECK((hipError_t)launch_book_device(d_hist, g.bklen, 0u, d_book, revbook, stream));
    return PSZ_SUCCESS;
  }
  g.eh = pend.hist_epoch;  // published by pass 1's last workgroup, or now
  if (!g.eh) {
    g.eh = ++epoch;
    CUSZ_AMD_HIP_CHECK((hipError_t)launch_publish(hist_regions(g.bklen), flag(kFlagHist), g.eh, stream));
  }
  g.eg = ++gate_epoch;
  g.armed = gate;
  if (!g.armed)
    if (int fs = g.build(twoqueue)) return fs;
  const XferRegions up = regions({{d_book, h_book(), (size_t)g.bklen * 4}, {revbook, h_revbook(), lay.rvbk}});
  if (g.armed)
    CUSZ_AMD_HIP_CHECK((hipError_t)launch_gate_upload(up, flag(kFlagGate), g.eg, timeout(), stream));
  else
    CUSZ_AMD_HIP_CHECK((hipError_t)launch_upload(up, stream));
  return PSZ_SUCCESS;
}

// the chunk tables and the bitstream of the archive's phf segment
Pipeline::PhfSections Pipeline::phf_sections(const PhfLayout& lay) const
{
  uint8_t* phf = d_archive + lay.phf_off;
  return {reinterpret_cast<uint32_t*>(phf + lay.nbit_rel), reinterpret_cast<uint32_t*>(phf + lay.entry_rel),
          reinterpret_cast<uint32_t*>(phf + lay.bits_rel)};
}

// a predictor's last workgroup publishes the histogram to the host (no publish launch)
HostPub Pipeline::hist_pub(int bklen) { return HostPub{hist_regions(bklen), flag(kFlagHist), ++epoch, hist_ticket()}; }

// a finish's last kernel publishes the summary finish_compress waits for (no publish launch)
HostPub Pipeline::summary_pub()
{
  return HostPub{readback_regions(), flag(kFlagSummary), summary_epoch = ++epoch, summary_ticket()};
}

// the histogram for the host codebook, and with a caller's reduced histogram its overflow word
XferRegions Pipeline::hist_regions(int bklen)
{
  XferRegions r = regions({{h_hist(), d_hist, (size_t)bklen * 4}, {&h_readback()->excess, d_hist + bklen, 4}});
  r.count = pend.ext ? 2 : 1;
  return r;
}

// header + summary; a sharded finish also reads back the word k_take_hist raises and the summed
// overflow word (the device-book path sends no histogram to the host)
XferRegions Pipeline::readback_regions()
{
  Readback* rb = h_readback();
  XferRegions r = regions({{rb->header, d_archive, sizeof(psz_header)}, {&rb->info, info(), sizeof(CompressInfo)},
                           {&rb->timeout, timeout(), pend.ext ? 12u : 8u}, {&rb->excess, d_hist + 2 * pend.radius, 4}});
  r.count = pend.ext ? 4 : 3;
  return r;
}

BrickCodes Pipeline::brick_codes(bool zz, int radius) const
{
  return BrickCodes{d_codes, d_codes8, d_rowmask, zz ? 0u : (uint32_t)std::max(radius - 127, 0)};
}

template <typename T>
int Pipeline::compress(psz_header* h, const T* in, uint8_t** out, size_t* outlen)
{
  if (broken) return PSZ_AMD_ERR_DEVICE;
  const psz_rc2 rc = h->rc;  // Rel mode scales eb in place: a second run starts from the caller's
  for (int run = 0;; run++) {
    const int g0 = grow_events;
    int s = compress_scan<T>(h, in, true);
    if (!s) s = compress_finish(h, nullptr, out, outlen, in);
    // bricks spilled past their slots (or past the spill list): the capacity has grown to hold
    // them, compress again (identical below the reference's 10 % cap, where this never runs)
    if (s != PSZ_WARN_OUTLIER_TOO_MANY || grow_events == g0 || run > 1) return s;
    h->rc = rc;
  }
}

// Pass 1: [extrema] -> predict + histogram + outliers (+ codes).  The histogram stays on the
// device (d_hist) for compress_finish, or for a caller that reduces it across slabs first.
// single: a single-process compress, whose finish follows with the scan's own histogram: the
// predictor publishes it (or its codebook sample) to the host itself (its last workgroup).
// Path::Stream: pass 1 is the sample kernel, which hands the histogram of every 16th 32 x 8 x 8
// unit to the host.
template <typename T>
int Pipeline::compress_scan(psz_header* h, const T* in, bool single)
{
  if (broken) return PSZ_AMD_ERR_DEVICE;
  pend.active = false;
  pend.ext = false;
  pend.side_book = false;
  const Choice c = choose_path(h, single);
  if (c.status) return c.status;
  const int radius = c.radius, bklen = c.bklen;
  const bool zz = c.zz, spl = c.path == Path::Spline, stream_mode = c.path == Path::Stream;
  const bool brick = c.path == Path::Brick || stream_mode;
  if (spl && !d_spl_slots) {  // spline outlier slots: one range per 32x8x8 tile, allocated on first use
    CUSZ_AMD_HIP_CHECK(d_spl_slots.alloc((size_t)sgeom.ntiles * spl_cap));
    CUSZ_AMD_HIP_CHECK(d_spl_cnt.alloc(sgeom.ntiles));
    CUSZ_AMD_HIP_CHECK(d_spl_off.alloc((size_t)sgeom.ntiles + 1));
    CUSZ_AMD_HIP_CHECK(d_spl_sps.alloc(sgeom.ntiles));
  }
  // chunk length: the caller's, else the tuned one
  if (!brick) {
    const int s = user_sublen ? std::min(8192, ((user_sublen + 255) / 256) * 256) : tuned_sublen;
    if (s != sublen) {
      sublen = s;
      pardeg = (int)((n - 1) / s + 1);
      CUSZ_AMD_HIP_CHECK(alloc_chunk_state());
    }
  }

  mark(kMarkBegin);
  if (int fs = scale_rel_eb<T>(h, in)) return fs;
  const double eb = h->rc.eb;

  // per-call state reset (the reference never resets these: SURVEY.md Appendix B.3); the brick
  // path's third region: pass 1's codebook sample.  The single pass: the sample, and the look-back
  // status words (one per brick), which live in the per-brick histogram area (unused in that mode)
  const std::tuple<void*, const void*, size_t> zh{d_hist, nullptr, (size_t)(bklen + 1) * 4}, zs{d_small, nullptr, kSmallZeroBytes},
      zb{d_shist, nullptr, ((size_t)kMaxBklen * kSampleBinStride + 16) * 4},
      zu{d_shist, nullptr, (size_t)kMaxBklen * kSampleBinStride * 4}, zl{d_bhist, nullptr, (size_t)bl.g.nbricks * 8};
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_zero(
      stream_mode ? regions({zu, zs, zl}) : brick ? regions({zh, zs, zb}) : regions({zh, zs}), stream));
  mark(kMarkExtrema);
  pend.path = c.path, pend.radius = radius, pend.zz = zz;
  pend.anchor_bytes = spl ? sizeof(T) * sgeom.anchor_len : 0;
  if (stream_mode) {
    // the sample histogram; its last workgroup publishes it to the host (kFlagHist)
    pend.hist_epoch = ++epoch;
    CUSZ_AMD_HIP_CHECK((hipError_t)launch_brick_sample<T>(bl, in, eb, radius, zz, d_shist, bklen, hist_ticket(), h_hist(),
                                                          flag(kFlagHist), pend.hist_epoch, stream));
  }
  else if (brick) {
    OutlierSink bol{d_slots, d_brick_cnt, d_spill, spill_cnt(), brick_slot_cap, spill_cap, nullptr};
    HostPub hp;
    const bool sampled_mode = codebook != PSZ_AMD_CODEBOOK_EXACT;
    BrickSample sample;
    if (sampled_mode && single && (bl.g.ndim == 3 || bl.g.ndim == 1)) {
      // a single-process compress: pass 1 visits a sample of the bricks first, counts them into
      // d_shist and hands the completed sample to the host, which builds the codebook (the
      // two-queue book of sample + 1) while pass 1 goes on; the encode launches wait behind
      // the device-polled gate as in the exact mode, but the book is ready long before
      sample = brick_sample_plan(bl, d_shist);
      sample.pub_dst = h_hist(), sample.pub_flag = flag(kFlagHist), sample.pub_epoch = ++epoch;
      pend.side_book = true;  // (the sample's epoch is pend.hist_epoch)
    }
    if (single && !pend.side_book) hp = hist_pub(bklen);  // (2-D bricks: the full histogram, as in the exact mode)
    pend.hist_epoch = pend.side_book ? sample.pub_epoch : hp.epoch;
    CUSZ_AMD_HIP_CHECK((hipError_t)launch_brick_scan<T>(bl, in, eb, radius, zz, sample, bol, d_hist, d_bhist,
                                                        brick_codes(zz, radius), bklen, stream, hp));
  }
  else if (spl) {
    OutlierSink ol{d_spl_slots, d_spl_cnt, d_spill, spill_cnt(), spl_cap, spill_cap, d_spl_sps};
    SplineArgs<T> sa{in, (uint32_t)len.x, (uint32_t)len.y, (uint32_t)len.z, sgeom.gdx, sgeom.gdy, sgeom.gdz, sgeom.ntiles,
                     (float)(1.0 / eb), (float)(eb * 2.0), radius, bklen, d_codes, reinterpret_cast<T*>(d_archive + 176), ol,
                     d_hist, &d_small.p->code_lost};
    pend.hist_epoch = 0;  // compress_finish publishes the histogram itself
    CUSZ_AMD_HIP_CHECK((hipError_t)launch_spline3_c<T>(sa, stream));
  }
  else {
    OutlierSink ol{d_slots, d_brick_cnt, d_spill, spill_cnt(), cap_per_brick, spill_cap, nullptr};
    // the kernel's last workgroup publishes the histogram to the host (no publish launch) for
    // the host's reference codebook (every mode: measured faster than the device book here)
    HostPub hp;
    if (single && c.path != Path::Fzg) hp = hist_pub(bklen);  // (FZG builds no book)
    pend.hist_epoch = hp.epoch;
    CUSZ_AMD_HIP_CHECK((hipError_t)launch_lorenzo_c<T>(in, len.x, len.y, len.z, eb, radius, zz, geom, d_codes,
                                                       ol, d_hist, bklen, stream, hp));
  }
  mark(kMarkPredict);
  pend.active = true;
  return PSZ_SUCCESS;
}

// Codebook (from d_hist, or from `ext_hist`: a device u32[bklen] the caller reduced across
// slabs) -> encode -> archive.  in: the field again, for the single pass (Path::Stream) only.
int Pipeline::compress_finish(psz_header* h, const uint32_t* ext_hist, uint8_t** out, size_t* outlen, const void* in)
{
  if (!pend.active) return PSZ_AMD_ERR_STATE;
  pend.active = false;
  pend.ext = ext_hist != nullptr;
  if (ext_hist) {
    // bklen counts + the summed overflow word of every slab (psz_amd_compress_scan_*).  FZG builds
    // no book (only the overflow word counts); every other path checks the counts against the
    // scan's own on the way in (k_take_hist), and finish_compress refuses a histogram that lacks
    // a bin this slab uses
    if (pend.path == Path::Fzg)
      CUSZ_AMD_HIP_CHECK(hipMemcpyAsync(d_hist, ext_hist, (size_t)(2 * pend.radius + 1) * 4, hipMemcpyDeviceToDevice, stream));
    else
      CUSZ_AMD_HIP_CHECK((hipError_t)launch_take_hist(ext_hist, d_hist, 2 * pend.radius, hist_missing(), stream));
    pend.hist_epoch = 0;  // the scan's published histogram is not the one to encode with
  }
  switch (pend.path) {
    case Path::Brick: return finish_brick(h, out, outlen);
    case Path::Fzg: return finish_fzg(h, out, outlen);
    case Path::Stream:
      return dtype == F4 ? finish_stream(h, static_cast<const float*>(in), out, outlen)
                         : finish_stream(h, static_cast<const double*>(in), out, outlen);
    default: return finish_huffman(h, out, outlen);  // Reference, Spline
  }
}

// Finalize of the index-order paths (Reference, Spline, Fzg): the scan of the outlier counts,
// which also writes both headers from their templates (static fields from the host, dynamic ones
// filled by the finalize workgroup, which knows the totals) -> the outlier copy -> the summary.
// seg_tpl: the phf_header, or (Fzg) the FzgHeader with the payload's 4-byte cells in the
// bitstream's role; data_rel: the bitstream's / payload's offset in the segment at seg_off.
int Pipeline::finalize_outliers(const psz_header* h, const void* seg_tpl, size_t seg_off, size_t data_rel,
                                const uint32_t* par_nbit, const uint32_t* par_entry, int npar)
{
  const bool spl = pend.path == Path::Spline, fzg = pend.path == Path::Fzg;
  const uint64_t* slots = spl ? d_spl_slots : d_slots;
  FinalizeArgs fa{par_nbit, par_entry, npar, spl ? d_spl_cnt : d_brick_cnt, spl ? sgeom.ntiles : geom.nbricks,
                  spl ? spl_cap : cap_per_brick, spill_cnt(), spill_cap, spl ? d_spl_off : d_brick_off, info(),
                  spl ? d_spl_sps.p : nullptr};
  fa.sizes_known = fzg;   // info()->total_ncell: the FZG encode's scan
  fa.nbit_known = !fzg;   // info()->total_nbit: the Huffman encoder's tile-sum pass
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_finalize_scan(fa, stream, h, seg_tpl, d_archive, seg_off, data_rel, fzg));
  OutlierCopyArgs oa{slots, fa.brick_cnt, fa.brick_off, fa.nbricks, fa.cap_per_brick, d_spill, spill_cnt(), spill_cap,
                     info(), d_archive, seg_off + data_rel, fa.spill_start};
  // the copy's last workgroup publishes the summary when its grid is small; a large grid pays the
  // publish per block, so a publish launch follows
  const HostPub sp = summary_pub();
  const bool in_copy = fa.nbricks <= 4096u;
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_outlier_copy(oa, stream, in_copy ? sp : HostPub{}));
  if (!in_copy) CUSZ_AMD_HIP_CHECK((hipError_t)launch_publish(sp.r, sp.flag, sp.epoch, stream));
  mark(kMarkFinalize);
  return PSZ_SUCCESS;
}

// Reference layout (Lorenzo or spline codes in index order).  Codebook: the reference's heap on
// the host (hf_hl.cc:21-34) when the predictor's last workgroup already published the histogram
// (Lorenzo, single process: config 1 book stage 9 us against 46 us for the device book), else --
// spline, a sharded finish -- on the device from the full histogram unless PSZ_AMD_CODEBOOK_EXACT
// (no host round trip).  On the host path, as in the brick path, every launch after the book is
// queued now behind a device-polled gate, and the last kernel publishes the summary: the
// histogram's trip to the host overlaps nothing, but no launch waits on the host's build.
int Pipeline::finish_huffman(psz_header* h, uint8_t** out, size_t* outlen)
{
  const int bklen = 2 * pend.radius;
  const PhfLayout lay(pend.anchor_bytes, bklen, (size_t)pardeg);
  BookGate book{*this, bklen};
  if (int fs = book_stage(book, false, lay)) return fs;
  mark(kMarkBook);

  const PhfSections ps = phf_sections(lay);
  HfEncodeArgs ea{d_codes, n, d_book, bklen, sublen, pardeg, ps.par_nbit, ps.par_entry, ps.bits, d_enc_temp,
                  plan_ticket(),          // (the brick plan's ticket: unused on this path)
                  &info()->total_nbit};   // summed by the encoder's tile-sum pass
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_hf_encode(ea, stream));
  mark(kMarkEncode);

  phf_header ph;
  fill_header_templates(lay, bklen, sublen, pardeg, n, len, h, &ph);
  if (int fs = finalize_outliers(h, &ph, lay.phf_off, lay.bits_rel, ea.par_nbit, ea.par_entry, pardeg)) return fs;
  if (int fs = book.build_if_armed(false)) return fs;
  return finish_compress(h, out, outlen);
}

// FZG finish: no codebook stage (the histogram is produced for psz_amd_compress_scan_*'s export
// and not used; of a caller's histogram only the overflow word counts) -> FZG encode into the
// archive -> finalize as on the Huffman path.
int Pipeline::finish_fzg(psz_header* h, uint8_t** out, size_t* outlen)
{
  mark(kMarkBook);
  const FzgLayout lay(n);
  uint8_t* seg = d_archive + lay.fzg_off;
  const uint32_t transform = pend.zz ? kFzgPlain : kFzgZigzagDelta;
  const FzgEncodeArgs ea{d_codes, n, pend.radius, transform, reinterpret_cast<uint64_t*>(seg + lay.flags_rel),
                         reinterpret_cast<uint32_t*>(seg + lay.off_rel), reinterpret_cast<uint64_t*>(seg + lay.payload_rel),
                         info()};
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_fzg_encode(ea, stream));
  mark(kMarkEncode);
  FzgHeader fh;
  fill_fzg_templates(lay, transform, len, h, &fh);
  if (int fs = finalize_outliers(h, &fh, lay.fzg_off, lay.payload_rel, nullptr, nullptr, 0)) return fs;
  return finish_compress(h, out, outlen);
}

// Fused brick compress (brick_scan.hip, brick_pack.hip): pass 1 (histograms + outliers) -> host codebook ->
// region reservation -> pass 2 (predict + pack straight into the archive) -> finalize.
int Pipeline::finish_brick(psz_header* h, uint8_t** out, size_t* outlen)
{
  const int radius = pend.radius, bklen = 2 * radius;
  const BrickGeom& g = bl.g;
  // The histogram goes to the host; the codebook comes back through host-mapped memory.  Every
  // launch after the codebook is queued NOW: the upload kernel polls a host-mapped gate word the
  // host sets once the book is built, so the encode kernels start right after it instead of
  // after the host's launch latency (and without the command processor's stream-wait latency).
  const PhfLayout lay(0, bklen, (size_t)g.nchunks);
  // host book: the reference heap on the full histogram (EXACT; 2-D bricks) or the two-queue
  // book of pass 1's sample + 1 (SAMPLED, published mid-pass); otherwise (a sharded finish: every
  // rank holds the same reduced histogram) the device book
  const bool sampled = pend.side_book;
  pend.side_book = false;
  BookGate book{*this, bklen};
  if (int fs = book_stage(book, sampled, lay)) return fs;
  mark(kMarkBook);

  // header templates: static fields from the host, sizes filled by the plan kernel
  phf_header ph;
  fill_header_templates(lay, bklen, g.W, (int)g.nchunks, n, len, h, &ph);

  const uint32_t nblk = brick_plan_blocks(g.nbricks);
  BrickPlanArgs pa{d_bhist, bklen, brick_hist_stride(bklen), d_book, g.nbricks, g.nbx, g.nby, bl.ly, bl.lz,
                   d_brick_cnt, brick_slot_cap, d_slots, d_spill, spill_cnt(), spill_cap, nblk, d_ub, d_bbase, d_brick_off,
                   d_plan, d_plan + nblk + 1, info(), d_archive, lay.phf_off, lay.bits_rel};
  pa.nd = g.ndim == 3 ? 3u : 1u, pa.nchunks = g.nchunks, pa.n = g.n;  // 1-D and 2-D: linear bricks
  pa.ticket = plan_ticket();
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_brick_plan(bl, pa, h, &ph, stream));
  const PhfSections ps = phf_sections(lay);
  // pass 2's last workgroup publishes the summary
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_brick_pack(bl, brick_codes(pend.zz, radius), d_book, bklen, pa, ps.par_nbit, ps.par_entry,
                                                   ps.bits, timeout(), stream, summary_pub()));
  mark(kMarkEncode);
  if (int fs = book.build_if_armed(sampled)) return fs;
  mark(kMarkFinalize);
  return finish_compress(h, out, outlen);
}

// Single-pass mode (PSZ_AMD_CODEBOOK_STREAM, 3-D bricks): the sample kernel (compress_scan) hands
// the histogram of every 16th 32 x 8 x 8 unit to the host, which builds the two-queue book of
// sample + 1 while the streaming pass predicts its first bricks; that pass takes the book behind
// a device-polled gate, sizes each brick (one workgroup per brick), takes its offset by a
// look-back and writes its rows straight to the archive; a finish kernel writes the outlier
// segment and the headers.  Codes, outliers and the reconstruction equal the exact mode's; the
// bitstream does not.
template <typename T>
int Pipeline::finish_stream(psz_header* h, const T* in, uint8_t** out, size_t* outlen)
{
  const int radius = pend.radius, bklen = 2 * radius;
  const BrickGeom& g = bl.g;
  // after the look-back status words (zeroed by the scan), the outlier count and destination of
  // each (brick, y-step) slot, all in the per-brick histogram area (2 KB a brick)
  unsigned long long* status = reinterpret_cast<unsigned long long*>(d_bhist.p);
  uint32_t* slot_cnt = reinterpret_cast<uint32_t*>(status + g.nbricks);
  uint32_t* slot_dst = slot_cnt + (size_t)g.nbricks * kStreamSlots;
  const PhfLayout lay(0, bklen, (size_t)g.nchunks);
  // the host's two-queue book of sample + 1 opens the gate the streaming pass polls (always
  // armed: CUSZ_AMD_NO_GATE only moves the build before the launch)
  BookGate book{*this, bklen, pend.hist_epoch, ++gate_epoch, true};
  if (!gate)  // (diagnostic switch: the book before the launch)
    if (int fs = book.build(true)) return fs;
  mark(kMarkBook);
  phf_header ph;
  fill_header_templates(lay, bklen, g.W, (int)g.nchunks, n, len, h, &ph);
  uint8_t* phf = d_archive + lay.phf_off;
  const PhfSections ps = phf_sections(lay);
  const size_t chunks = std::max((size_t)pardeg, (size_t)g.nchunks);
  BrickSingle sg{OutlierSink{d_slots, slot_cnt, d_spill, spill_cnt(), brick_slot_cap / kStreamSlots, spill_cap, nullptr},
                 d_book, bklen, ps.par_nbit, ps.par_entry, ps.bits,
                 (uint32_t)std::min<size_t>(bitstream_cells_cap() + chunks, 0xFFFFFFFFu),
                 status, &info()->ticket, slot_dst, info(), timeout(), d_archive, lay.phf_off, lay.bits_rel,
                 flag(kFlagGate), book.eg, h_book(), reinterpret_cast<const uint32_t*>(h_revbook()),
                 reinterpret_cast<uint32_t*>(phf + lay.rvbk_rel), (int)(lay.rvbk / 4), book_flag()};
  CUSZ_AMD_HIP_CHECK((hipError_t)launch_brick_stream<T>(bl, in, h->rc.eb, radius, pend.zz, sg, h, &ph, stream, summary_pub()));
  mark(kMarkEncode);
  mark(kMarkFinalize);
  if (int fs = book.build_if_armed(true)) return fs;
  return finish_compress(h, out, outlen);
}

// read back the device-written header + summary (one flag wait), report status
int Pipeline::finish_compress(psz_header* h, uint8_t** out, size_t* outlen)
{
  if (int fs = wait_flag(kFlagSummary, summary_epoch)) return fs;  // (every finish's last kernel: summary_pub)
  if (timing) CUSZ_AMD_HIP_CHECK(hipEventSynchronize(ev[kMarkFinalize]));
  const Readback* rb = h_readback();
  CompressInfo ci;
  std::memcpy(&ci, &rb->info, sizeof(ci));
  unsigned int tmo;
  std::memcpy(&tmo, &rb->timeout, 4);
  std::memcpy(h, rb->header, sizeof(psz_header));
  splen = (size_t)ci.splen;
  const bool spl = pend.path == Path::Spline;
  if (timing) {
    stage_ms[PSZ_AMD_T_EXTREMA] = span(kMarkBegin, kMarkExtrema);
    stage_ms[PSZ_AMD_T_PREDICT] = span(kMarkExtrema, kMarkPredict);
    stage_ms[PSZ_AMD_T_BOOK] = pend.path == Path::Fzg ? 0.f : span(kMarkPredict, kMarkBook);  // FZG: no codebook stage
    stage_ms[PSZ_AMD_T_ENCODE] = span(kMarkBook, kMarkEncode);
    stage_ms[PSZ_AMD_T_FINALIZE] = span(kMarkEncode, kMarkFinalize);
    stage_ms[PSZ_AMD_T_COMPRESS] = span(kMarkBegin, kMarkFinalize);
  }
  if (tmo) {
    std::fprintf(stderr, "[cusz_amd] encoder reservation/look-back check failed\n");
    return PSZ_AMD_ERR_ENCODER;
  }
  // the caller's histogram had a zero bin for a symbol this slab uses (a wrong reduction): the
  // encode ran on a book that gives that symbol weight 1, and its archive is not handed out
  if (pend.ext && rb->hist_missing) {
    pend.ext = false;
    return PSZ_AMD_ERR_INVALID_ARG;
  }
  // spline: some point's code is past what an outlier cell carries (cusz_amd.h): decompression
  // could not reproduce the compressor's codes, so no archive is handed back
  if (spl && rb->code_lost) return PSZ_AMD_ERR_CODE_RANGE;
  if (ci.spilled && !spl) {
    // bricks spilled past their slots: grow the slots to the largest brick's count so that the
    // repeat writes every cell in its brick's slot (deterministic order, fused decoders' ranked
    // reads); compress() then runs once more, a scan/finish caller gets the warning and repeats
    const int g = grow_slots(ci.max_brick_cnt);
    if (g < 0) return PSZ_AMD_ERR_DEVICE;
    if (g > 0) return PSZ_WARN_OUTLIER_TOO_MANY;
  }
  if (ci.outlier_lost) {
    // the spill list was too small for this field's outliers (every cell was counted): grow it
    // (and the archive) to hold them all; compress() then runs once more, a scan/finish caller
    // gets the warning and repeats scan and finish
    const int g = grow_spill((uint64_t)spill_cap + ci.outlier_lost);
    if (g < 0) return PSZ_AMD_ERR_DEVICE;
    return PSZ_WARN_OUTLIER_TOO_MANY;
  }
  // a sharded finish: another slab overflowed (the summed overflow word), so every rank sees
  // the warning and repeats the step together
  const uint32_t gx = pend.ext ? rb->excess : 0u;
  pend.ext = false;  // consumed: a later call never reads this finish's overflow word
  if (gx) return PSZ_WARN_OUTLIER_TOO_MANY;
  *out = d_archive;
  *outlen = h->entry[PSZHEADER_ENC_PASS2_END];
  return PSZ_SUCCESS;
}

template int Pipeline::compress<float>(psz_header*, const float*, uint8_t**, size_t*);
template int Pipeline::compress<double>(psz_header*, const double*, uint8_t**, size_t*);
template int Pipeline::compress_scan<float>(psz_header*, const float*, bool);
template int Pipeline::compress_scan<double>(psz_header*, const double*, bool);

}  // namespace cusz_amd
