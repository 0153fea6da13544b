// cusz_amd/csrc/api_rev1.cc -- the C API over the Pipeline (pipeline.hh): the resource manager of
// cusz_rev1.h, the extensions of cusz_amd.h (scan / finish, regions, quality, knobs) and the
// pszheader_* / phf_* helpers.  Argument checks and the header's bookkeeping live here: first the
// typed bodies, then every exported function.  The older per-call API of cusz.h is api_legacy.cc,
// on top of this one.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

#include "cusz.h"
#include "hf.h"
#include "pipeline.hh"

using cusz_amd::Pipeline;

static Pipeline* P(psz_resource* m) { return m ? reinterpret_cast<Pipeline*>(m->buf) : nullptr; }

static thread_local int g_create_status = PSZ_SUCCESS;  // psz_amd_last_create_status

static psz_resource* make_resource(psz_header* hdr, void* stream)
{
  g_create_status = PSZ_AMD_ERR_DEVICE;  // allocation failures below
  auto* m = new (std::nothrow) psz_resource;
  if (!m) return nullptr;
  std::memset(m, 0, sizeof(*m));
  m->header = hdr;
  m->len_linear = hdr->len.x * hdr->len.y * hdr->len.z;
  m->stream = stream;
  m->device = AMDGPU;
  m->dict_size = (uint16_t)(hdr->rc.radius * 2);
  auto* p = new (std::nothrow) Pipeline;
  if (!p) {
    delete m;
    return nullptr;
  }
  int st = p->init(hdr->dtype, hdr->len, stream);
  g_create_status = st;
  m->buf = p;
  m->ndim = p->ndim;
  m->last_error = (psz_error_status)st;
  if (st != PSZ_SUCCESS) {
    delete p;
    delete hdr;
    delete m;
    return nullptr;
  }
  return m;
}

// What a compress and a scan do before the pipeline runs: the type check, the radius clamp
// (*warn = PSZ_WARN_RADIUS_TOO_LARGE, the status of a call that otherwise succeeds), the header's
// error-bound fields and the device.
template <typename T>
static int begin_compress(psz_resource* m, psz_rc2 rc, const T* in, int* warn)
{
  if (!m || !in) return PSZ_AMD_ERR_INVALID_ARG;
  if ((sizeof(T) == 4) != (m->header->dtype == F4)) return PSZ_ABORT_UNSUPPORTED_TYPE;
  *warn = PSZ_SUCCESS;
  if (rc.radius > 512) rc.radius = 512, *warn = PSZ_WARN_RADIUS_TOO_LARGE;  // libcusz.cc:281-285
  m->header->rc = rc;
  m->header->user_input_eb = rc.eb;
  // the value range is this call's (Rel mode) or none: the reference leaves the previous call's
  // range in the header (libcusz.cc:287-293 writes it only in Rel mode), so an Abs archive's
  // bytes would depend on the manager's history (per-call state reset)
  m->header->min_val = m->header->max_val = 0;
  m->dict_size = (uint16_t)(rc.radius * 2);
  CUSZ_AMD_HIP_CHECK(hipSetDevice(P(m)->device));  // the creation device (B.7; several GPUs per process)
  return PSZ_SUCCESS;
}

template <typename T>
static int compress_impl(psz_resource* m, psz_rc2 rc, T* in, psz_header* out_h, uint8_t** out, size_t* outlen)
{
  if (!out || !outlen) return PSZ_AMD_ERR_INVALID_ARG;
  int warn;
  if (const int s = begin_compress<T>(m, rc, in, &warn)) return s;
  const int s = P(m)->compress<T>(m->header, in, out, outlen);
  if (out_h) *out_h = *m->header;
  return s != PSZ_SUCCESS ? s : warn;
}

template <typename T>
static int scan_impl(psz_resource* m, psz_rc2 rc, T* in)
{
  int warn;
  if (const int s = begin_compress<T>(m, rc, in, &warn)) return s;
  const int s = P(m)->compress_scan<T>(m->header, in);
  return s != PSZ_SUCCESS ? s : warn;
}

// scan, then the slab histogram (device) to the caller's device buffer, on the manager's stream
template <typename T>
static int scan_export(psz_resource* m, psz_rc2 rc, T* in, uint32_t* d_out)
{
  const int status = scan_impl<T>(m, rc, in);
  if (status != PSZ_SUCCESS && status != PSZ_WARN_RADIUS_TOO_LARGE) return status;
  Pipeline* p = P(m);
  if (!d_out) return PSZ_AMD_ERR_INVALID_ARG;
  const int bklen = 2 * m->header->rc.radius;
  CUSZ_AMD_HIP_CHECK(hipMemcpyAsync(d_out, p->d_hist, sizeof(uint32_t) * bklen, hipMemcpyDeviceToDevice, p->stream));
  // word bklen: this slab's spilled outlier cells -- past its bricks' slots (Lorenzo: every rank
  // then repeats with grown slots, deterministic archives) or past its spill list (spline) --
  // summed with the histograms
  const uint32_t free_spill = p->pend.path == cusz_amd::Path::Spline ? p->spill_cap : 0u;
  CUSZ_AMD_HIP_CHECK((hipError_t)cusz_amd::launch_excess(p->spill_cnt(), free_spill, d_out + bklen, p->stream));
  return status;
}

// Quality assessment (include/cusz_amd.h): one pass + one combine launch on the manager's stream,
// one wait for the 232-byte record, the struct finished on the host (quality_reduce.hh).  Touches
// no compress or decompress state.  box: field extents, origin, extent (the region variant).
template <typename T>
static int assess_quality_impl(psz_resource* m, const T* x, const T* o, size_t len, const psz_len* box, double eb,
                               int flags, psz_amd_quality* out)
{
  Pipeline* p = P(m);
  if (!p || !x || !o || !out || !(eb >= 0.0) || (flags & ~PSZ_AMD_QUALITY_AUTOCOR)) return PSZ_AMD_ERR_INVALID_ARG;
  if (box) {
    if (!cusz_amd::box_inside(box[0], box[1], box[2])) return PSZ_AMD_ERR_INVALID_ARG;
    len = box[2].x * box[2].y * box[2].z;
  }
  if (len == 0) return PSZ_AMD_ERR_INVALID_ARG;
  CUSZ_AMD_HIP_CHECK(hipSetDevice(p->device));
  if (!p->d_quality) CUSZ_AMD_HIP_CHECK(p->d_quality.alloc(cusz_amd::kQrGridCap + 1));
  const bool ac = (flags & PSZ_AMD_QUALITY_AUTOCOR) != 0;
  const double thr = eb > 0.0 ? 1.001 * eb : INFINITY;
  if (box) {
    const size_t o3[3] = {box[1].x, box[1].y, box[1].z}, e3[3] = {box[2].x, box[2].y, box[2].z};
    CUSZ_AMD_HIP_CHECK((hipError_t)cusz_amd::launch_quality_region<T>(x, o, box[0].x, box[0].y, o3, e3, thr, ac,
                                                                       p->d_quality, p->stream));
  }
  else
    CUSZ_AMD_HIP_CHECK((hipError_t)cusz_amd::launch_quality<T>(x, o, len, thr, ac, p->d_quality, p->stream));
  cusz_amd::QrPart part;
  CUSZ_AMD_HIP_CHECK(hipMemcpyAsync(&part, p->d_quality.p + cusz_amd::kQrGridCap, sizeof(part), hipMemcpyDeviceToHost,
                                    p->stream));
  CUSZ_AMD_HIP_CHECK(hipStreamSynchronize(p->stream));
  cusz_amd::qr_to_quality(part, len, eb, ac, out);
  return PSZ_SUCCESS;
}

// What a decompress and a region decode do first: the header's segment table must be ordered and
// fit the archive the caller passed; then the type check and the device.
template <typename T>
static int begin_decompress(psz_resource* m, const uint8_t* in, size_t in_len, const T* out)
{
  if (!m || !in || !out) return PSZ_AMD_ERR_INVALID_ARG;
  const uint32_t* e = m->header->entry;
  for (int k = 1; k <= PSZHEADER_ENC_PASS2_END; k++)
    if (e[k] < e[k - 1]) return PSZ_AMD_ERR_BAD_ARCHIVE;
  if (in_len && e[PSZHEADER_ENC_PASS2_END] > in_len) return PSZ_AMD_ERR_BAD_ARCHIVE;
  if ((size_t)e[PSZHEADER_ENC_PASS1_END] - e[PSZHEADER_SPFMT] != 8 * m->header->splen) return PSZ_AMD_ERR_BAD_ARCHIVE;
  if ((sizeof(T) == 4) != (m->header->dtype == F4)) return PSZ_ABORT_UNSUPPORTED_TYPE;
  CUSZ_AMD_HIP_CHECK(hipSetDevice(P(m)->device));
  return PSZ_SUCCESS;
}

template <typename T>
static int decompress_impl(psz_resource* m, uint8_t* in, size_t in_len, T* out)
{
  if (const int c = begin_decompress<T>(m, in, in_len, out)) return c;
  Pipeline* p = P(m);
  const int s = p->decompress<T>(m->header, in, out);
  if (s == PSZ_SUCCESS && p->timing) p->collect_decompress_times();
  return s;
}

template <typename T>
static int decompress_region_impl(psz_resource* m, uint8_t* in, size_t in_len, psz_len o, psz_len e, T* out)
{
  if (const int c = begin_decompress<T>(m, in, in_len, out)) return c;
  return P(m)->decompress_region<T>(m->header, in, o, e, out);
}

extern "C" {

// =========================================================================================
// resource-manager API (cusz_rev1.h)
// =========================================================================================

psz_resource* psz_create_resource_manager(psz_dtype dtype, psz_len len, psz_pipeline pipeline, void* stream)
{
  g_create_status = PSZ_ABORT_UNSUPPORTED_TYPE;
  if (dtype != F4 && dtype != F8) return nullptr;
  g_create_status = PSZ_AMD_ERR_DEVICE;
  auto* h = new (std::nothrow) psz_header;
  if (!h) return nullptr;
  std::memset(h, 0, sizeof(*h));
  h->dtype = dtype;
  h->pipeline = pipeline;
  h->len = len;
  h->rc.radius = DEFAULT_RADIUS;
  h->intp_param = make_default_params();
  auto* m = make_resource(h, stream);
  if (m) phf_coarse_tune(m->len_linear, &h->vle_sublen, &h->vle_pardeg);
  return m;
}

psz_resource* psz_create_resource_manager_from_header(psz_header* header, void* stream)
{
  g_create_status = !header ? PSZ_AMD_ERR_INVALID_ARG : PSZ_ABORT_UNSUPPORTED_TYPE;
  if (!header || (header->dtype != F4 && header->dtype != F8)) return nullptr;
  g_create_status = PSZ_AMD_ERR_DEVICE;
  auto* h = new (std::nothrow) psz_header;
  if (!h) return nullptr;
  std::memcpy(h, header, sizeof(psz_header));
  return make_resource(h, stream);
}

void psz_modify_resource_manager_from_header(psz_resource* m, psz_header* header)
{
  if (!m || !header) return;
  std::memcpy(m->header, header, sizeof(psz_header));
  m->dict_size = (uint16_t)(m->header->rc.radius * 2);
  m->len_linear = header->len.x * header->len.y * header->len.z;
}

int psz_release_resource(psz_resource* m)
{
  if (!m) return PSZ_SUCCESS;
  delete P(m);
  delete m->cli;
  delete m->header;
  delete m;
  return PSZ_SUCCESS;
}

int psz_compress_float(psz_resource* m, psz_rc2 rc, float* in, psz_header* out_h, uint8_t** out, size_t* outlen)
{
  return compress_impl<float>(m, rc, in, out_h, out, outlen);
}

int psz_compress_double(psz_resource* m, psz_rc2 rc, double* in, psz_header* out_h, uint8_t** out,
                        size_t* outlen)
{
  return compress_impl<double>(m, rc, in, out_h, out, outlen);
}

int psz_compress_analyize_float(psz_resource* m, psz_rc2 rc, float* in, u4* exported_h_hist)
{
  // compressor.inl:305-337: predict + histogram only, the histogram exported to the host
  if (!exported_h_hist) return PSZ_AMD_ERR_INVALID_ARG;
  const int s = scan_impl<float>(m, rc, in);
  if (s != PSZ_SUCCESS && s != PSZ_WARN_RADIUS_TOO_LARGE) return s;
  Pipeline* p = P(m);
  const size_t bytes = sizeof(u4) * 2 * m->header->rc.radius;
  const int fs = p->fetch(Pipeline::regions({{p->h_hist(), p->d_hist, bytes}}), cusz_amd::kFlagHist);
  p->pend.active = false;
  if (fs) return fs;
  std::memcpy(exported_h_hist, p->h_hist(), bytes);
  return s;
}

int psz_decompress_float(psz_resource* m, uint8_t* in, size_t const in_len, float* out)
{
  return decompress_impl<float>(m, in, in_len, out);
}

int psz_decompress_double(psz_resource* m, uint8_t* in, size_t const in_len, double* out)
{
  return decompress_impl<double>(m, in, in_len, out);
}

// =========================================================================================
// extensions (cusz_amd.h)
// =========================================================================================

int psz_amd_compress_scan_float(psz_resource* m, psz_rc2 rc, float* in, uint32_t* d_hist_out)
{
  return scan_export<float>(m, rc, in, d_hist_out);
}

int psz_amd_compress_scan_double(psz_resource* m, psz_rc2 rc, double* in, uint32_t* d_hist_out)
{
  return scan_export<double>(m, rc, in, d_hist_out);
}

int psz_amd_compress_finish(psz_resource* m, const uint32_t* d_hist, psz_header* out_h, uint8_t** out,
                            size_t* outlen)
{
  Pipeline* p = P(m);
  if (!p || !out || !outlen) return PSZ_AMD_ERR_INVALID_ARG;
  CUSZ_AMD_HIP_CHECK(hipSetDevice(p->device));
  const int s = p->compress_finish(m->header, d_hist, out, outlen);
  if (out_h) *out_h = *m->header;
  return s;
}

int psz_amd_value_range(psz_resource* m, const void* in, size_t len, double* d_minmax)
{
  Pipeline* p = P(m);
  if (!p || !in || !d_minmax) return PSZ_AMD_ERR_INVALID_ARG;
  if (len == 0) len = p->n;
  CUSZ_AMD_HIP_CHECK(hipSetDevice(p->device));
  if (m->header->dtype == F4)
    CUSZ_AMD_HIP_CHECK((hipError_t)cusz_amd::launch_extrema<float>(static_cast<const float*>(in), len, d_minmax,
                                                                   p->ext_scratch(), p->stream));
  else
    CUSZ_AMD_HIP_CHECK((hipError_t)cusz_amd::launch_extrema<double>(static_cast<const double*>(in), len, d_minmax,
                                                                    p->ext_scratch(), p->stream));
  return PSZ_SUCCESS;
}

int psz_amd_assess_quality_float(psz_resource* m, const float* x, const float* o, size_t len, double eb, int flags,
                                 psz_amd_quality* out)
{
  return assess_quality_impl<float>(m, x, o, len, nullptr, eb, flags, out);
}

int psz_amd_assess_quality_double(psz_resource* m, const double* x, const double* o, size_t len, double eb, int flags,
                                  psz_amd_quality* out)
{
  return assess_quality_impl<double>(m, x, o, len, nullptr, eb, flags, out);
}

int psz_amd_assess_quality_region_float(psz_resource* m, const float* xbox, const float* ofield, psz_len field_len,
                                        psz_len origin, psz_len extent, double eb, int flags, psz_amd_quality* out)
{
  const psz_len box[3] = {field_len, origin, extent};
  return assess_quality_impl<float>(m, xbox, ofield, 0, box, eb, flags, out);
}

int psz_amd_assess_quality_region_double(psz_resource* m, const double* xbox, const double* ofield, psz_len field_len,
                                         psz_len origin, psz_len extent, double eb, int flags, psz_amd_quality* out)
{
  const psz_len box[3] = {field_len, origin, extent};
  return assess_quality_impl<double>(m, xbox, ofield, 0, box, eb, flags, out);
}

int psz_amd_region_plan(const psz_header* h, psz_len origin, psz_len extent, psz_amd_region_info* out)
{
  return psz_amd_region_plan_mode(h, origin, extent, PSZ_AMD_REGION_MODE_WHOLE, out);
}

int psz_amd_region_plan_mode(const psz_header* h, psz_len origin, psz_len extent, int mode, psz_amd_region_info* out)
{
  if (!h || !out) return PSZ_AMD_ERR_INVALID_ARG;
  return cusz_amd::region_plan(h, origin, extent, mode, out);
}

int psz_amd_set_region_mode(psz_resource* m, int mode)
{
  Pipeline* p = P(m);
  if (!p || (mode != PSZ_AMD_REGION_MODE_WHOLE && mode != PSZ_AMD_REGION_MODE_COVER)) return PSZ_AMD_ERR_INVALID_ARG;
  p->region_mode = mode;
  return PSZ_SUCCESS;
}

int psz_amd_decompress_region_float(psz_resource* m, uint8_t* in, size_t in_len, psz_len origin, psz_len extent,
                                    float* out)
{
  return decompress_region_impl<float>(m, in, in_len, origin, extent, out);
}

int psz_amd_decompress_region_double(psz_resource* m, uint8_t* in, size_t in_len, psz_len origin, psz_len extent,
                                     double* out)
{
  return decompress_region_impl<double>(m, in, in_len, origin, extent, out);
}

int psz_amd_last_region(psz_resource* m, psz_amd_region_info* out)
{
  Pipeline* p = P(m);
  if (!p || !out) return PSZ_AMD_ERR_INVALID_ARG;
  if (!p->has_last_region) return PSZ_AMD_ERR_STATE;
  *out = p->last_region;
  return PSZ_SUCCESS;
}

int psz_amd_get_internals(psz_resource* m, psz_amd_internals* o)
{
  Pipeline* p = P(m);
  if (!p || !o) return PSZ_AMD_ERR_INVALID_ARG;
  o->d_quant_codes = p->d_codes;
  o->d_hist = p->d_hist;
  o->d_book = p->d_book;
  o->len = p->n;
  o->bklen = 2 * m->header->rc.radius;
  o->sublen = p->sublen;
  o->pardeg = p->pardeg;
  o->ndim = p->ndim;
  o->splen = p->splen;
  o->archive_capacity = p->archive_cap;
  o->layout = p->last_layout();
  o->brick_width = p->bl.g.ok ? p->bl.g.W : 0;
  return PSZ_SUCCESS;
}

int psz_amd_enable_timing(psz_resource* m, int on)
{
  Pipeline* p = P(m);
  if (!p) return PSZ_AMD_ERR_INVALID_ARG;
  p->timing = on != 0;
  return PSZ_SUCCESS;
}

int psz_amd_stage_times(psz_resource* m, float* ms, int n)
{
  Pipeline* p = P(m);
  if (!p || !ms) return PSZ_AMD_ERR_INVALID_ARG;
  for (int i = 0; i < n && i < PSZ_AMD_T_COUNT; i++) ms[i] = p->stage_ms[i];
  return PSZ_SUCCESS;
}

int psz_amd_set_sublen(psz_resource* m, int sublen)
{
  Pipeline* p = P(m);
  if (!p || sublen < 0) return PSZ_AMD_ERR_INVALID_ARG;
  p->user_sublen = sublen;
  if (sublen == 0) {
    cusz_amd::tune_chunking(p->n, p->device, &p->sublen, &p->pardeg);
    if (p->alloc_chunk_state() != hipSuccess) return PSZ_AMD_ERR_DEVICE;
  }
  return PSZ_SUCCESS;
}

int psz_amd_set_decoder(psz_resource* m, int kind)
{
  Pipeline* p = P(m);
  if (!p || kind < PSZ_AMD_DECODER_AUTO || kind > PSZ_AMD_DECODER_WAVE) return PSZ_AMD_ERR_INVALID_ARG;
  p->decoder = kind;
  return PSZ_SUCCESS;
}

int psz_amd_set_codebook(psz_resource* m, int mode)
{
  Pipeline* p = P(m);
  if (!p || (mode != PSZ_AMD_CODEBOOK_EXACT && mode != PSZ_AMD_CODEBOOK_SAMPLED && mode != PSZ_AMD_CODEBOOK_STREAM))
    return PSZ_AMD_ERR_INVALID_ARG;
  p->codebook = mode;
  return PSZ_SUCCESS;
}

int psz_amd_set_layout(psz_resource* m, int layout)
{
  Pipeline* p = P(m);
  if (!p) return PSZ_AMD_ERR_INVALID_ARG;
  if (layout != PSZ_AMD_LAYOUT_BRICK && layout != PSZ_AMD_LAYOUT_REFERENCE && layout != PSZ_AMD_LAYOUT_BRICK_FORCE)
    return PSZ_AMD_ERR_INVALID_ARG;
  p->layout = layout == PSZ_AMD_LAYOUT_REFERENCE ? PSZ_AMD_LAYOUT_REFERENCE : PSZ_AMD_LAYOUT_BRICK;
  p->layout_set = layout == PSZ_AMD_LAYOUT_BRICK_FORCE;  // BRICK keeps the small-2-D default
  return PSZ_SUCCESS;
}

int psz_amd_decode_codes(psz_resource* m, uint8_t* in)
{
  Pipeline* p = P(m);
  if (!p || !in) return PSZ_AMD_ERR_INVALID_ARG;
  return p->decode_codes(m->header, in);
}

const char* psz_amd_version(void) { return "cusz_amd 0.1 (gfx950)"; }

int psz_amd_last_create_status(void) { return g_create_status; }

int psz_amd_build_book_device(const uint32_t* IN_d_hist, int bklen, uint32_t smooth, uint32_t* OUT_d_book,
                              uint8_t* OUT_d_revbook, void* stream)
{
  if (!IN_d_hist || !OUT_d_book || !OUT_d_revbook || bklen < 1 || bklen > 1024) return PSZ_AMD_ERR_INVALID_ARG;
  CUSZ_AMD_HIP_CHECK((hipError_t)cusz_amd::launch_book_device(IN_d_hist, bklen, smooth, OUT_d_book, OUT_d_revbook,
                                                                (hipStream_t)stream));
  return PSZ_SUCCESS;
}

// internal: the older API passes a stream per call (cusz.h psz_compress/psz_decompress)
int cusz_amd_set_stream(psz_resource* m, void* stream)
{
  Pipeline* p = P(m);
  if (!p) return PSZ_AMD_ERR_INVALID_ARG;
  p->stream = (hipStream_t)stream;
  m->stream = stream;
  return PSZ_SUCCESS;
}

// =========================================================================================
// header / phf helpers (psz/src/utils/header.c:9-30, codec/hf/src/libphf.cc:26-76)
// =========================================================================================

psz_len pszheader_len(psz_header* h) { return h->len; }
size_t pszheader_len_linear(psz_header* h) { return h->len.x * h->len.y * h->len.z; }
size_t pszheader_segments(psz_header*) { return sizeof(psz_header); }
size_t pszheader_filesize(psz_header* h) { return h->entry[PSZHEADER_ENC_PASS2_END]; }
size_t pszheader_uncompressed_len(psz_header* h) { return pszheader_len_linear(h); }
size_t pszheader_compressed_bytes(psz_header* h) { return pszheader_filesize(h); }

uint32_t phf_encoded_bytes(phf_header* h) { return h->entry[PHFHEADER_END]; }

size_t phf_coarse_tune_sublen(size_t len)
{
  int s, p;
  phf_coarse_tune(len, &s, &p);
  return (size_t)s;
}

void phf_coarse_tune(size_t len, int* sublen, int* pardeg)
{
  int dev = 0;
  (void)hipGetDevice(&dev);
  cusz_amd::tune_chunking(len, dev, sublen, pardeg);
}

size_t phf_reverse_book_bytes(u2 bklen, size_t BK_UNIT_BYTES, size_t SYM_BYTES)
{
  return BK_UNIT_BYTES * (2 * BK_UNIT_BYTES * 8) + SYM_BYTES * bklen;
}

void phf_version(void) { std::printf("\n///  cusz_amd HF (gfx950) build\n"); }
void phf_versioninfo(void) { phf_version(); }

}  // extern "C"
