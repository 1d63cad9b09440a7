// capi_stage.h -- the stage entry points of include/hesaff_amd.h (hesaff_stage_*: one operator of the pipeline on the caller's data) and
// the arena their device arrays live in.  Included at the end of pipeline.hip, behind capi_impl.h (same translation unit: needs
// hesaff_ctx, the launchers and capi_impl.h's HS_API_BEGIN / HS_API_END, bind_device and finish_stream).
#pragma once

namespace {

// The device arrays of one stage call, in the context's stage buffer: declare them (add<T>(count), StagePlan of buffer_layouts.h: each
// 256-byte aligned), ensure() once, then address, fill and read them by array.  Every copy goes to the main stream, in call order.
struct StageArena : StagePlan {
   hesaff_ctx *c;
   explicit StageArena(hesaff_ctx *ctx) : c(ctx) {}
   void ensure() { c->b_stage.ensure(bytes()); }
   template <class T> T *ptr(const Span<T> &a) const { return c->b_stage.at<T>(a.off); }
   template <class T> void upload(const Span<T> &a, const T *src) { HIP_TRY(hipMemcpyAsync(ptr(a), src, a.bytes(), hipMemcpyHostToDevice, c->stream())); }
   template <class T> void download(T *dst, const Span<T> &a) { HIP_TRY(hipMemcpyAsync(dst, ptr(a), a.bytes(), hipMemcpyDeviceToHost, c->stream())); }
   template <class T> void zero(const Span<T> &a) { HIP_TRY(hipMemsetAsync(ptr(a), 0, a.bytes(), c->stream())); }
};

// hesaff_detect_batch_device_f32's check (k_check_f32) of n planes in device memory, before any kernel reads them as an image: one flag
// per image, read back once; a refused image is copied back to name its first pixel outside the domain
void check_device_f32(hesaff_ctx *c, int n, const uint8_t *d, long long img_stride, int row_stride, int H, int W)
{
   StageArena a(c);
   const Span<int32_t> flags = a.add<int32_t>((size_t)n);
   a.ensure();
   a.zero(flags);
   const int gx = std::max(1, std::min(H, (8 * c->n_cu + n - 1) / n));   // about 8 blocks per CU in all
   hipLaunchKernelGGL(k_check_f32, dim3(gx, 1, n), dim3(256), 0, c->stream(), d, img_stride, row_stride, H, W, a.ptr(flags));
   std::vector<int32_t> h((size_t)n);
   a.download(h.data(), flags);
   finish_stream(c);
   for (int b = 0; b < n; b++) {
      if (!h[(size_t)b]) continue;
      std::vector<uint8_t> img((size_t)H * W * 4);
      HIP_TRY(hipMemcpy2D(img.data(), (size_t)W * 4, d + (long long)b * img_stride, (size_t)row_stride, (size_t)W * 4, (size_t)H, hipMemcpyDeviceToHost));
      throw_bad_f32(b, img.data(), H, W, (size_t)W * 4);
   }
}

} // namespace

extern "C" {

// ---------------------------------- stage entry points ----------------------------------

// The stage entry points run the PRODUCTION kernels wherever the batch path has one for the operator:
//   gaussianBlur     -> k_blur_hess_march<K> (K = 9, 11, 13, 15: every blur of the default pyramid), else the generic two-pass kernels
//   hessianResponse  -> the fused R0 epilogue of k_blur_hess_march<9, .., WRITE_R0> (pyramid.cpp:230 on the batch path)
//   SIFT             -> k_sift_meanvar / _grad / _hist (histogram, then normalise / clip / quantise)
//   normalizeAffine  -> k_prepare_patch + the five window-size bin kernels
//   findAffineShape  -> hs_affine_groups (k_affine's body)
// halfImage has no stand-alone production kernel (the decimation is an epilogue of the K = 13 blur launch, checked
// plane by plane through hesaff_stage_pyramid); k_half serves the operator here.
int hesaff_stage_gaussian_blur(hesaff_ctx *c, const float *in, int rows, int cols, float sigma, float *out)
{
   if (!c || !in || !out || rows < 1 || cols < 1 || !(sigma > 0.0f)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   const int K = hesaff::gauss_ksize(sigma);
   const int pitch = round_up(cols, 64);   // like the batch planes: rows stay 16-byte aligned for the float4 stores
   const size_t n = (size_t)rows * pitch;
   StageArena a(c);
   const Span<float> a_in = a.add<float>(n), a_tmp = a.add<float>(n), a_out = a.add<float>(n), a_taps = a.add<float>((size_t)K);
   a.ensure();
   float *d_in = a.ptr(a_in), *d_tmp = a.ptr(a_tmp), *d_out = a.ptr(a_out), *d_taps = a.ptr(a_taps);
   std::vector<float> taps(K);
   hesaff::blur_taps(K, sigma, taps.data());
   HIP_TRY(hipMemcpy2DAsync(d_in, (size_t)pitch * 4, in, (size_t)cols * 4, (size_t)cols * 4, rows, hipMemcpyHostToDevice, c->stream()));
   a.upload(a_taps, taps.data());
   DPlane pi = make_plane(d_in, rows, cols, pitch), pt = make_plane(d_tmp, rows, cols, pitch), po = make_plane(d_out, rows, cols, pitch);
   const DPlane none = make_plane(nullptr, 0, 0, 0);
   if (K == 1) {
      HIP_TRY(hipMemcpyAsync(d_out, d_in, n * 4, hipMemcpyDeviceToDevice, c->stream()));
   } else if (K == 9 || K == 11 || K == 13 || K == 15) {
      launch_blur_hess<true, false, false>(c, pi, po, none, none, d_taps, K, 0.0f, 1);
   } else {
      const dim3 grid((cols + 255) / 256, rows, 1);
      hipLaunchKernelGGL(k_blur_rows_generic, grid, dim3(256), 0, c->stream(), pi, pt, (const float *)d_taps, K);
      hipLaunchKernelGGL(k_blur_cols_generic, grid, dim3(256), 0, c->stream(), pt, po, (const float *)d_taps, K);
   }
   HIP_TRY(hipMemcpy2DAsync(out, (size_t)cols * 4, d_out, (size_t)pitch * 4, (size_t)cols * 4, rows, hipMemcpyDeviceToHost, c->stream()));
   finish_stream(c);
   HS_API_END(c)
}

int hesaff_stage_hessian_response(hesaff_ctx *c, const float *in, int rows, int cols, float norm, float *out)
{
   if (!c || !in || !out || rows < 1 || cols < 1) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   const int pitch = round_up(cols, 64);
   const size_t n = (size_t)rows * pitch;
   StageArena a(c);
   const Span<float> a_in = a.add<float>(n), a_out = a.add<float>(n), a_l = a.add<float>(n), a_r = a.add<float>(n), a_taps = a.add<float>(9);
   a.ensure();
   float *d_in = a.ptr(a_in), *d_out = a.ptr(a_out), *d_l = a.ptr(a_l), *d_r = a.ptr(a_r), *d_taps = a.ptr(a_taps);
   HIP_TRY(hipMemcpy2DAsync(d_in, (size_t)pitch * 4, in, (size_t)cols * 4, (size_t)cols * 4, rows, hipMemcpyHostToDevice, c->stream()));
   DPlane pi = make_plane(d_in, rows, cols, pitch), po = make_plane(d_out, rows, cols, pitch);
   // the batch path computes R0 in the epilogue of the first blur launch of an octave (K = 9 at the default sigmas)
   std::vector<float> taps(9);
   hesaff::blur_taps(9, hesaff::make_schedule(1.6f, false).blur_sigma[1], taps.data());
   a.upload(a_taps, taps.data());
   launch_march<9, true, true, false, true>(c, pi, make_plane(d_l, rows, cols, pitch), make_plane(d_r, rows, cols, pitch), make_plane(nullptr, 0, 0, 0),
                                            d_taps, 1.0f, 1, po, norm * norm);
   HIP_TRY(hipMemcpy2DAsync(out, (size_t)cols * 4, d_out, (size_t)pitch * 4, (size_t)cols * 4, rows, hipMemcpyDeviceToHost, c->stream()));
   finish_stream(c);
   HS_API_END(c)
}

int hesaff_stage_half_image(hesaff_ctx *c, const float *in, int rows, int cols, float *out)
{
   if (!c || !in || !out || rows < 2 || cols < 2) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   const size_t n = (size_t)rows * cols;
   const int r2 = rows / 2, c2 = cols / 2;
   StageArena a(c);
   const Span<float> a_in = a.add<float>(n), a_out = a.add<float>((size_t)r2 * c2);
   a.ensure();
   a.upload(a_in, in);
   DPlane pi = make_plane(a.ptr(a_in), rows, cols, cols), po = make_plane(a.ptr(a_out), r2, c2, c2);
   hipLaunchKernelGGL(k_half, dim3((c2 + 255) / 256, r2, 1), dim3(256), 0, c->stream(), pi, po);
   a.download(out, a_out);
   finish_stream(c);
   HS_API_END(c)
}

// hesaff_stage_pyramid and its float twin: `image` is rows x cols pixels of 1 byte or, f32, of 4, tightly packed.  Out come all
// planes of every octave, L0..L4 then R0..R4, without pitch padding: the builder's, with L4 kept in a scratch plane sized here
static int stage_pyramid(hesaff_ctx *c, const void *image, bool f32, int rows, int cols, float *planes, int *n_octaves, size_t *n_floats)
{
   if (!c || rows < 1 || cols < 1) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   plan(c, 1, rows, cols);
   size_t nf = 0;
   for (const OctGeom &g : c->oct) nf += (size_t)10 * g.rows * g.cols;
   if (n_octaves) *n_octaves = (int)c->oct.size();
   if (n_floats) *n_floats = nf;
   if (planes) {
      if (!image) throw HsError(HESAFF_ERR_ARG, f32 ? "plane is NULL" : "gray is NULL");
      const size_t row_bytes = (size_t)cols * (f32 ? 4 : 1), bytes = row_bytes * rows;
      if (f32) {
         if ((uintptr_t)image % 4 != 0) throw HsError(HESAFF_ERR_ARG, "float plane not 4-byte aligned");
         int r = 0, col = 0;
         float v = 0.0f;
         if (first_bad_f32((const uint8_t *)image, rows, cols, row_bytes, &r, &col, &v))   // the value domain of the _f32 entry points
            throw_bad_f32(0, (const uint8_t *)image, rows, cols, row_bytes);
      }
      c->b_input.ensure(bytes);
      if (!c->oct.empty()) c->b_stage.ensure((size_t)c->oct[0].rows * c->oct[0].pitch * 4);   // L4 of the largest octave, the plan's first
      HIP_TRY(hipMemcpyAsync(c->b_input.p, image, bytes, hipMemcpyHostToDevice, c->stream()));
      c->ev_used = 0;
      StageTimer tm(c);
      const SrcImages src = f32 ? SrcImages::f32(c->b_input.p, (long long)bytes, (int)row_bytes) : SrcImages::u8(c->b_input.p, 1, (long long)bytes, (int)row_bytes);
      build_first_level(c, src, 1, tm);
      float *pout = planes;
      for (size_t o = 0; o < c->oct.size(); o++) {
         const OctGeom &g = c->oct[o];
         OctavePlanes P = octave_planes(c, o, 1);
         P.L[4] = make_plane(c->b_stage.as<float>(), g.rows, g.cols, g.pitch);
         build_octave(c, o, 1, P, OctaveWant::DetectKeepL4, tm);
         // (before the next octave overwrites L3 and the response planes: the copies are in stream order)
         for (int l = 0; l < 10; l++, pout += (size_t)g.rows * g.cols)
            HIP_TRY(hipMemcpy2DAsync(pout, (size_t)g.cols * 4, (l < 5 ? P.L[l] : P.R[l - 5]).p, (size_t)g.pitch * 4, (size_t)g.cols * 4, g.rows, hipMemcpyDeviceToHost,
                                     c->stream()));
      }
      finish_stream(c);
   }
   HS_API_END(c)
}

int hesaff_stage_pyramid(hesaff_ctx *c, const uint8_t *gray, int rows, int cols, float *planes, int *n_octaves, size_t *n_floats)
{
   return stage_pyramid(c, gray, false, rows, cols, planes, n_octaves, n_floats);
}

int hesaff_stage_pyramid_f32(hesaff_ctx *c, const float *plane, int rows, int cols, float *planes, int *n_octaves, size_t *n_floats)
{
   return stage_pyramid(c, plane, true, rows, cols, planes, n_octaves, n_floats);
}

// the first m entries of the ordered Hessian list as the stage entry points return them (image: optional)
static void fetch_hessian_list(hesaff_ctx *c, const Lists &s, int m, float *f, int32_t *iv, int32_t *image)
{
   std::vector<float> x(m), y(m), sc(m), resp(m);
   std::vector<int32_t> meta(m), key(m);
   HIP_TRY(hipMemcpy(x.data(), s.hl.x, (size_t)m * 4, hipMemcpyDeviceToHost));
   HIP_TRY(hipMemcpy(y.data(), s.hl.y, (size_t)m * 4, hipMemcpyDeviceToHost));
   HIP_TRY(hipMemcpy(sc.data(), s.hl.s, (size_t)m * 4, hipMemcpyDeviceToHost));
   HIP_TRY(hipMemcpy(resp.data(), s.hl.response, (size_t)m * 4, hipMemcpyDeviceToHost));
   HIP_TRY(hipMemcpy(meta.data(), s.hl.meta, (size_t)m * 4, hipMemcpyDeviceToHost));
   HIP_TRY(hipMemcpy(key.data(), s.hl.r0c0, (size_t)m * 4, hipMemcpyDeviceToHost));
   for (int i = 0; i < m; i++) {
      const int octave = (meta[i] >> 4) & 15, level = (meta[i] >> 2) & 3, type = meta[i] & 3;
      const OctGeom &g = c->oct[octave];
      const uint32_t pix = (uint32_t)key[i] % (uint32_t)(g.rows * g.cols);
      f[5 * i] = x[i]; f[5 * i + 1] = y[i]; f[5 * i + 2] = sc[i]; f[5 * i + 3] = c->ct.consts.pd0 * (float)(1 << octave); f[5 * i + 4] = resp[i];
      iv[5 * i] = type; iv[5 * i + 1] = octave; iv[5 * i + 2] = level; iv[5 * i + 3] = (int32_t)(pix / g.cols); iv[5 * i + 4] = (int32_t)(pix % g.cols);
      if (image) image[i] = meta[i] >> 8;
   }
}

// the end of a stage operator that has enqueued detection: waits, refuses a list that did not fit, returns its length and first `cap` entries
static void finish_hessian_list(hesaff_ctx *c, const Lists &s, int cap, float *f, int32_t *iv, int32_t *image, int *count)
{
   CounterHead cn;
   HIP_TRY(hipMemcpyAsync(&cn, &s.counters->head, sizeof cn, hipMemcpyDeviceToHost, c->stream()));
   finish_stream(c);
   if (cn.overflow != 0 || cn.rec > c->cap) throw HsError(HESAFF_ERR_CAPACITY, "keypoint capacity exceeded");
   *count = (int)cn.hess_total;
   const int m = std::min(*count, cap);
   if (m > 0 && f && iv) fetch_hessian_list(c, s, m, f, iv, image);
}

int hesaff_stage_hessian_keypoints(hesaff_ctx *c, const uint8_t *gray, int rows, int cols, int cap, float *f, int32_t *iv, int *count)
{
   if (!c || !gray || rows < 1 || cols < 1 || !count) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   plan(c, 1, rows, cols);
   c->b_input.ensure((size_t)rows * cols);
   HIP_TRY(hipMemcpyAsync(c->b_input.p, gray, (size_t)rows * cols, hipMemcpyHostToDevice, c->stream()));
   c->ev_used = 0;
   StageTimer tm(c);
   Lists s = make_lists(c);
   run_detection(c, SrcImages::u8(c->b_input.p, 1, (long long)rows * cols, cols), 1, s, tm);
   finish_hessian_list(c, s, cap, f, iv, nullptr, count);
   HS_API_END(c)
}

// The detection chain on the caller's planes: what run_detection does with an octave's planes once it has made them (begin_detection,
// detect_octave, order_hessian_list: pipeline.hip), on octave 0 of a plan for n_images x rows x cols.
int hesaff_stage_detect_planes(hesaff_ctx *c, int n_images, int rows, int cols, const float *L, const float *R, int band, int cap, float *f,
                               int32_t *iv, int32_t *image, int *count)
{
   const int min_size = 2 * HS_BORDER + 2;   // pyramid.cpp:283: the smallest plane that is an octave
   if (!c || !L || !R || !count || n_images < 1 || rows <= min_size || cols <= min_size) return HESAFF_ERR_ARG;
   if (band != 0 && band != 32 && band != 64 && band != 128) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (c->ct.up) throw HsError(HESAFF_ERR_ARG, "hesaff_stage_detect_planes: the planes are the first pyramid level as given; not with upscaleInputImage");
   plan(c, n_images, rows, cols);
   const OctGeom &g = c->oct[0];
   hipStream_t st = c->stream();
   const size_t tight = (size_t)rows * cols;
   const OctavePlanes P = octave_planes(c, 0, n_images);
   // cols floats per row: the pitch padding behind them keeps what it held.  k_extrema_march's clamped 16-byte loads read it, as they do on
   // the batch path (the blur kernels store cols floats too); it can only reach columns that are not scanned
   for (int b = 0; b < n_images; b++)
      for (int l = 0; l < 5; l++) {
         const size_t off = ((size_t)b * 5 + l) * tight;
         HIP_TRY(hipMemcpy2DAsync(P.R[l].img(b), (size_t)g.pitch * 4, R + off, (size_t)cols * 4, (size_t)cols * 4, rows, hipMemcpyHostToDevice, st));
         if (l < 4) HIP_TRY(hipMemcpy2DAsync(P.L[l].img(b), (size_t)g.pitch * 4, L + off, (size_t)cols * 4, (size_t)cols * 4, rows, hipMemcpyHostToDevice, st));
      }
   c->ev_used = 0;
   StageTimer tm(c);
   Lists s = make_lists(c);
   begin_detection(c, s, n_images);
   detect_octave(c, s, tm, n_images, 0, P.L, P.R, band);
   order_hessian_list(c, s, tm, n_images);
   finish_hessian_list(c, s, cap, f, iv, image, count);
   HS_API_END(c)
}

int hesaff_stage_find_affine_shape(hesaff_ctx *c, const float *blur, int rows, int cols, int n, const float *kp, int32_t *converged,
                                   float *U, int32_t *iters)
{
   if (!c || !blur || !kp || rows < 2 || cols < 2 || n < 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t np = (size_t)rows * cols;
   const size_t N = (size_t)n;
   StageArena a(c);
   const Span<float> a_plane = a.add<float>(np), a_kp = a.add<float>(4 * N);
   const Span<int32_t> a_conv = a.add<int32_t>(N), a_iters = a.add<int32_t>(N);
   const Span<float> a_U = a.add<float>(4 * N);
   a.ensure();
   a.upload(a_plane, blur);
   a.upload(a_kp, kp);
   AffineOut ao; ao.converged = a.ptr(a_conv); ao.iters = a.ptr(a_iters); ao.U = a.ptr(a_U);
   DPlane P = make_plane(a.ptr(a_plane), rows, cols, cols);
   hipLaunchKernelGGL(k_affine_stage, dim3(std::min((n + HS_AFF_SLOTS - 1) / HS_AFF_SLOTS, 256 * 6)), dim3(64), 0, c->stream(), P, (const float *)a.ptr(a_kp), n, c->tables.view, c->ct.consts, ao);
   if (converged) a.download(converged, a_conv);
   if (iters) a.download(iters, a_iters);
   if (U) a.download(U, a_U);
   finish_stream(c);
   HS_API_END(c)
}

int hesaff_stage_rectify(hesaff_ctx *c, int n, float *A)
{
   if (!c || !A || n < 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   StageArena a(c);
   const Span<float> a_A = a.add<float>((size_t)n * 4);
   a.ensure();
   a.upload(a_A, (const float *)A);
   hipLaunchKernelGGL(k_rectify_stage, dim3((n + 255) / 256), dim3(256), 0, c->stream(), n, a.ptr(a_A));
   a.download(A, a_A);
   finish_stream(c);
   HS_API_END(c)
}

// hs_affine_tail (k_affine's tail: kernels_keypoint.h) on caller-supplied operands, with the context's convergenceThreshold
int hesaff_stage_affine_tail(hesaff_ctx *c, int n, float *abc, float *U, float *ratio, float *l, int32_t *state)
{
   if (!c || n < 0 || (n > 0 && (!abc || !U || !ratio || !l || !state))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t N = (size_t)n;
   StageArena a(c);
   const Span<float> a_abc = a.add<float>(3 * N), a_U = a.add<float>(4 * N), a_ratio = a.add<float>(N), a_l = a.add<float>(4 * N);
   const Span<int32_t> a_state = a.add<int32_t>(N);
   a.ensure();
   a.upload(a_abc, (const float *)abc);
   a.upload(a_U, (const float *)U);
   a.upload(a_ratio, (const float *)ratio);
   hipLaunchKernelGGL(k_affine_tail_stage, dim3((n + 255) / 256), dim3(256), 0, c->stream(), n, c->ct.consts.convergenceThreshold, a.ptr(a_abc), a.ptr(a_U),
                      a.ptr(a_ratio), a.ptr(a_l), a.ptr(a_state));
   a.download(abc, a_abc);
   a.download(U, a_U);
   a.download(ratio, a_ratio);
   a.download(l, a_l);
   a.download(state, a_state);
   finish_stream(c);
   HS_API_END(c)
}

// normalizeAffine for caller-supplied keypoints: reuses the batch kernels through a
// one-image plan whose Hessian list is filled from the arguments.
int hesaff_stage_normalize_affine(hesaff_ctx *c, const float *img, int rows, int cols, int n, const float *kp, const float *A,
                                  int32_t *rejected, float *patches)
{
   if (!c || !img || !kp || !A || rows < 2 || cols < 2 || n < 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   plan(c, 1, rows, cols);
   if ((uint32_t)n > c->cap) throw HsError(HESAFF_ERR_CAPACITY, "too many keypoints for this image size");
   Lists s = make_lists(c);
   hipStream_t st = c->stream();
   HIP_TRY(hipMemcpy2DAsync(c->gray.p, (size_t)c->gray.pitch * 4, img, (size_t)cols * 4, (size_t)cols * 4, rows, hipMemcpyHostToDevice, st));
   std::vector<float> x(n), y(n), sc(n);
   std::vector<int32_t> meta(n, 0), P0(n), alive(n);
   for (int i = 0; i < n; i++) { x[i] = kp[3 * i]; y[i] = kp[3 * i + 1]; sc[i] = kp[3 * i + 2]; }
   HIP_TRY(hipMemcpyAsync(s.hl.x, x.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemcpyAsync(s.hl.y, y.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemcpyAsync(s.hl.s, sc.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemcpyAsync(s.hl.meta, meta.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
   // feed A through the affine-output slot as an already rectified matrix: k_prepare_patch
   // would rectify again, so do its arithmetic (mrScale, P0, border test) via a dedicated kernel
   HIP_TRY(hipMemcpyAsync(s.pw.A, A, (size_t)n * 16, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemsetAsync(s.counters, 0, sizeof(CounterBlock), st));
   uint32_t nn = (uint32_t)n;
   HIP_TRY(hipMemcpyAsync(&s.counters->head.hess_total, &nn, 4, hipMemcpyHostToDevice, st));
   hipLaunchKernelGGL(k_prepare_patch_given_A, dim3((n + 255) / 256), dim3(256), 0, st, s.hl, (const uint32_t *)&s.counters->head.hess_total, rows, cols,
                      c->ct.consts, c->tables.view, s.pw);
   c->b_patches.ensure((size_t)n * HS_PATCH_PIX * 4);
   HIP_TRY(hipMemsetAsync(c->b_patches.p, 0, (size_t)n * HS_PATCH_PIX * 4, st));
   // T' rows of the huge windows: bounded by the sum of their sides
   const LargeRows lr = host_large_rows(sc.data(), n, c->ct.consts.mrSize, c->tables.view.max_p0);
   c->batch_max_p = lr.max_p;
   run_patch_stage(c, s, c->gray, c->b_patches.as<float>(), 0, lr.rows);
   uint32_t ovf = 0;
   HIP_TRY(hipMemcpyAsync(&ovf, &s.counters->head.row_overflow, 4, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipMemcpyAsync(alive.data(), s.pw.alive, (size_t)n * 4, hipMemcpyDeviceToHost, st));
   if (patches) HIP_TRY(hipMemcpyAsync(patches, c->b_patches.p, (size_t)n * HS_PATCH_PIX * 4, hipMemcpyDeviceToHost, st));
   finish_stream(c);
   if (ovf) throw HsError(HESAFF_ERR_NOMEM, "large-window row buffer exceeded (internal bound violated)");
   if (rejected) for (int i = 0; i < n; i++) rejected[i] = alive[i] ? 0 : 1;
   HS_API_END(c)
}

// hesaff_stage_sift and hesaff_stage_sift_parts: the production descriptor kernels on caller-supplied patches; meanvar / hist
// (either may be null) additionally receive what k_sift_meanvar left in the stage buffer and the histogram k_sift_hist writes out
// when it is given a place for it (SiftIO::vec; the pipeline passes none)
// alive (may be null: every keypoint alive): the pipeline's flags; desc then goes to the device first (dead keypoints' rows stay)
// desc_mode: the operator's own (stage operators do not read the context's modes)
static int stage_sift(hesaff_ctx *c, int n, const float *patches, float *meanvar, float *hist, uint8_t *desc, const int32_t *alive = nullptr,
                      int desc_mode = HESAFF_DESC_SIFT)
{
   if (!c || !patches || !desc || n < 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t N = (size_t)n;
   const GroupScratch gs = group_scratch((uint32_t)n);   // the patches, mean / variance and gradient pairs as the pipeline sizes them
   StageArena a(c);
   const Span<float> a_patches = a.add<float>(gs.patch_floats);
   const Span<int32_t> a_alive = a.add<int32_t>(N);
   const Span<float> a_mv = a.add<float>(gs.meanvar_floats), a_vec = a.add<float>(N * 128);
   const Span<uint8_t> a_desc = a.add<uint8_t>(N * 128);
   const Span<float> a_vo = a.add<float>(gs.vo_floats);
   a.ensure();
   std::vector<int32_t> ones(N, 1);
   a.upload(a_patches, patches);
   a.upload(a_alive, alive ? alive : ones.data());
   if (alive) a.upload(a_desc, (const uint8_t *)desc);
   a.zero(a_vo);   // pairs outside the circular mask stay (0, 0)
   SiftIO so;
   so.patches = a.ptr(a_patches); so.alive = a.ptr(a_alive); so.meanvar = a.ptr(a_mv);
   so.vec = hist ? a.ptr(a_vec) : nullptr; so.desc = a.ptr(a_desc); so.h_lo = 0; so.h_hi = (uint32_t)n;
   launch_sift(c, c->stream(), so, (uint32_t)n, (float2 *)a.ptr(a_vo), desc_mode);
   if (meanvar) a.download(meanvar, a_mv);
   if (hist) a.download(hist, a_vec);
   a.download(desc, a_desc);
   finish_stream(c);
   HS_API_END(c)
}

int hesaff_stage_sift(hesaff_ctx *c, int n, const float *patches, uint8_t *desc) { return stage_sift(c, n, patches, nullptr, nullptr, desc); }

int hesaff_stage_sift_parts(hesaff_ctx *c, int n, const float *patches, float *meanvar, float *hist, uint8_t *desc)
{
   if (!meanvar || !hist) return HESAFF_ERR_ARG;
   return stage_sift(c, n, patches, meanvar, hist, desc);
}

int hesaff_stage_sift_alive(hesaff_ctx *c, int n, const float *patches, const int32_t *alive, uint8_t *desc)
{
   if (!alive) return HESAFF_ERR_ARG;
   return stage_sift(c, n, patches, nullptr, nullptr, desc, alive);
}

int hesaff_stage_sift_mode(hesaff_ctx *c, int n, const float *patches, const int32_t *alive, int mode, uint8_t *desc)
{
   if (mode != HESAFF_DESC_SIFT && mode != HESAFF_DESC_ROOTSIFT) return HESAFF_ERR_ARG;
   return stage_sift(c, n, patches, nullptr, nullptr, desc, alive, mode);
}

// k_orientation (kernels_orient.h) on caller-supplied patches: every keypoint alive, no affine frame to turn
int hesaff_stage_orientation(hesaff_ctx *c, int n, const float *patches, float *theta, float *hist, float *cs)
{
   if (!c || !patches || !theta || n < 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t N = (size_t)n;
   StageArena a(c);
   const Span<float> a_patches = a.add<float>(N * HS_PATCH_PIX), a_theta = a.add<float>(N), a_hist = a.add<float>(N * HS_ORI_BINS), a_cs = a.add<float>(N * 2);
   a.ensure();
   a.upload(a_patches, patches);
   OrientIO oi;
   memset(&oi, 0, sizeof oi);
   oi.patches = a.ptr(a_patches); oi.h_lo = 0; oi.h_hi = (uint32_t)n;
   oi.theta = a.ptr(a_theta); oi.hist = a.ptr(a_hist); oi.cs = a.ptr(a_cs);
   hipLaunchKernelGGL(k_orientation, dim3(orientation_grid(c, (uint32_t)n)), dim3(64), 0, c->stream(), oi, c->tables.view);
   a.download(theta, a_theta);
   if (hist) a.download(hist, a_hist);
   if (cs) a.download(cs, a_cs);
   finish_stream(c);
   HS_API_END(c)
}

// k_orientation_peaks on caller-supplied patches: every keypoint alive, no frame to turn, no rank arrays
int hesaff_stage_orientation_peaks(hesaff_ctx *c, int n, const float *patches, int k, int32_t *n_ori, int32_t *bins, float *theta)
{
   if (!c || !patches || !n_ori || !bins || !theta || n < 0 || k < 1 || k > HS_ORI_MAX_COUNT) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t N = (size_t)n;
   StageArena a(c);
   const Span<float> a_patches = a.add<float>(N * HS_PATCH_PIX);
   const Span<int32_t> a_n = a.add<int32_t>(N), a_bins = a.add<int32_t>(N * HS_ORI_MAX_COUNT);
   const Span<float> a_theta = a.add<float>(N * HS_ORI_MAX_COUNT);
   a.ensure();
   a.upload(a_patches, patches);
   HIP_TRY(hipMemsetAsync(a.ptr(a_n), 0, a.bytes() - a_n.off, c->stream()));   // the three outputs, which end the arena
   OrientIO oi;
   memset(&oi, 0, sizeof oi);
   oi.patches = a.ptr(a_patches); oi.h_lo = 0; oi.h_hi = (uint32_t)n;
   OrientRanks mr;
   memset(&mr, 0, sizeof mr);
   mr.K = k; mr.n_ori = a.ptr(a_n); mr.bins = a.ptr(a_bins); mr.thetas = a.ptr(a_theta);
   hipLaunchKernelGGL(k_orientation_peaks, dim3(orientation_grid(c, (uint32_t)n)), dim3(64), 0, c->stream(), oi, c->tables.view, mr);
   // (an orientation count below 4 leaves the ranks beyond it to the host: bin -1, angle 0)
   a.download(n_ori, a_n);
   a.download(bins, a_bins);
   a.download(theta, a_theta);
   finish_stream(c);
   for (size_t i = 0; i < N; i++)
      for (int j = k; j < HS_ORI_MAX_COUNT; j++) { bins[i * HS_ORI_MAX_COUNT + j] = -1; theta[i * HS_ORI_MAX_COUNT + j] = 0.0f; }
   HS_API_END(c)
}

// exportKeypoints on the device for caller-supplied records: the kernels hesaff_process_files runs per chunk
int hesaff_stage_export(hesaff_ctx *c, const hesaff_keypoint *keys, int n, float mrSize, int format, char **out, size_t *len)
{
   if (!c || n < 0 || (n > 0 && !keys) || !out || !len || (format != HESAFF_OUT_TEXT && format != HESAFF_OUT_BIN)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   const float saved = c->par.mrSize;
   c->par.mrSize = mrSize;
   char *buf = nullptr;
   try {
      const size_t N = (size_t)n;
      c->b_stage.ensure(std::max<size_t>(N * sizeof(KeyRec), 16));
      if (n > 0) HIP_TRY(hipMemcpyAsync(c->b_stage.p, keys, N * sizeof(KeyRec), hipMemcpyHostToDevice, c->stream()));
      const KeyRec *d_keys = c->b_stage.as<KeyRec>();
      char head[64];
      size_t hl, body;
      if (format == HESAFF_OUT_TEXT) {
         const int32_t starts[2] = {0, n};
         c->b_ex_starts.ensure(16);
         HIP_TRY(hipMemcpyAsync(c->b_ex_starts.p, starts, sizeof starts, hipMemcpyHostToDevice, c->stream()));
         std::vector<unsigned long long> off;
         body = (size_t)export_text_prepare(c, d_keys, (uint32_t)n, c->b_ex_starts.as<int32_t>(), 1, off);
         hl = (size_t)snprintf(head, sizeof head, "%d\n%d\n", 128, n);
      } else {
         body = N * EX_BIN_ROW;
         memcpy(head, "HESAFFB1", 8);
         const uint32_t dim = 128, cnt = (uint32_t)n;
         memcpy(head + 8, &dim, 4); memcpy(head + 12, &cnt, 4);
         hl = 16;
      }
      buf = (char *)malloc(hl + body + 1);
      if (!buf) throw HsError(HESAFF_ERR_NOMEM, "malloc failed");
      memcpy(buf, head, hl);
      if (body > 0) {
         c->b_generic.ensure(body + 16);
         if (format == HESAFF_OUT_TEXT) export_text_write(c, d_keys, (uint32_t)n, (char *)c->b_generic.p);
         else export_bin_rows(c, d_keys, (uint32_t)n, (char *)c->b_generic.p);
         HIP_TRY(hipMemcpyAsync(buf + hl, c->b_generic.p, body, hipMemcpyDeviceToHost, c->stream()));
      }
      finish_stream(c);
      *out = buf;
      *len = hl + body;
   } catch (...) {
      c->par.mrSize = saved;
      free(buf);
      throw;
   }
   c->par.mrSize = saved;
   HS_API_END(c)
}

int hesaff_stage_fmt_g(hesaff_ctx *c, int n, const float *v, char *text, int32_t *lens)
{
   if (!c || n < 0 || (n > 0 && (!v || !text || !lens))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t N = (size_t)n;
   StageArena a(c);
   const Span<float> a_v = a.add<float>(N);
   const Span<int32_t> a_len = a.add<int32_t>(N);
   const Span<char> a_text = a.add<char>(N * 16);
   a.ensure();
   a.upload(a_v, v);
   a.zero(a_text);
   hipLaunchKernelGGL(k_fmt_g_test, dim3((n + 255) / 256), dim3(256), 0, c->stream(), n, (const float *)a.ptr(a_v), a.ptr(a_text), a.ptr(a_len));
   a.download(text, a_text);
   a.download(lens, a_len);
   finish_stream(c);
   HS_API_END(c)
}

int hesaff_stage_jpeg_pixels(hesaff_ctx *c, const hesaff_jpeg_layout *layout, int n, const uint8_t *blobs, size_t blob_bytes, uint8_t *pixels)
{
   if (!c || !layout || n < 0 || (n > 0 && (!blobs || !pixels))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const JpegGeom g = make_jpeg_geom(*layout);
   if ((size_t)g.blob_bytes != blob_bytes) throw HsError(HESAFF_ERR_ARG, "blob size does not match the layout");
   const size_t img = (size_t)g.W * g.H * g.nc;
   DevBuf &b_jcoef = c->slot[0].b_jcoef;   // (no chunk is on its way during a stage call)
   b_jcoef.ensure(blob_bytes * (size_t)n);
   c->b_stage.ensure(img * (size_t)n);
   HIP_TRY(hipMemcpyAsync(b_jcoef.p, blobs, blob_bytes * (size_t)n, hipMemcpyHostToDevice, c->stream()));
   jpeg_pixels(c, b_jcoef.as<uint8_t>(), g, n, c->b_stage.as<uint8_t>(), img, c->stream());
   HIP_TRY(hipMemcpyAsync(pixels, c->b_stage.p, img * (size_t)n, hipMemcpyDeviceToHost, c->stream()));
   finish_stream(c);
   HS_API_END(c)
}

int hesaff_stage_math(hesaff_ctx *c, int n, const float *a, const float *b, float *atan2_out, float *pow2_out)
{
   if (!c || !a || !b || n < 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t N = (size_t)n;
   StageArena ar(c);
   const Span<float> a_a = ar.add<float>(N), a_b = ar.add<float>(N), a_at = ar.add<float>(N), a_pw = ar.add<float>(N);
   ar.ensure();
   ar.upload(a_a, a);
   ar.upload(a_b, b);
   hipLaunchKernelGGL(k_math, dim3((n + 255) / 256), dim3(256), 0, c->stream(), n, (const float *)ar.ptr(a_a), (const float *)ar.ptr(a_b), ar.ptr(a_at), ar.ptr(a_pw));
   if (atan2_out) ar.download(atan2_out, a_at);
   if (pow2_out) ar.download(pow2_out, a_pw);
   finish_stream(c);
   HS_API_END(c)
}

int hesaff_stage_math_sift(hesaff_ctx *c, int n, const float *gy, const float *gx, float *ori_general, float *ori_nd, float *grad_general,
                           float *grad_nd)
{
   if (!c || !gy || !gx || !ori_general || !ori_nd || !grad_general || !grad_nd || n < 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t N = (size_t)n;
   StageArena a(c);
   const Span<float> a_gy = a.add<float>(N), a_gx = a.add<float>(N), a_out[4] = {a.add<float>(N), a.add<float>(N), a.add<float>(N), a.add<float>(N)};
   a.ensure();
   a.upload(a_gy, gy);
   a.upload(a_gx, gx);
   hipLaunchKernelGGL(k_math_sift, dim3(std::min(4096, (n + 255) / 256)), dim3(256), 0, c->stream(), n, (const float *)a.ptr(a_gy), (const float *)a.ptr(a_gx),
                      a.ptr(a_out[0]), a.ptr(a_out[1]), a.ptr(a_out[2]), a.ptr(a_out[3]));
   float *outs[4] = {ori_general, ori_nd, grad_general, grad_nd};
   for (int q = 0; q < 4; q++) a.download(outs[q], a_out[q]);
   finish_stream(c);
   HS_API_END(c)
}

int hesaff_stage_math_sift_general(hesaff_ctx *c, int n, const float *gy, const float *gx, float *ori, float *grad, float *coord)
{
   if (!c || !gy || !gx || !ori || !grad || !coord || n < 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t N = (size_t)n;
   StageArena a(c);
   const Span<float> a_gy = a.add<float>(N), a_gx = a.add<float>(N), a_out[3] = {a.add<float>(N), a.add<float>(N), a.add<float>(N)};
   a.ensure();
   a.upload(a_gy, gy);
   a.upload(a_gx, gx);
   hipLaunchKernelGGL(k_math_sift_general, dim3(std::min(4096, (n + 255) / 256)), dim3(256), 0, c->stream(), n, (const float *)a.ptr(a_gy),
                      (const float *)a.ptr(a_gx), a.ptr(a_out[0]), a.ptr(a_out[1]), a.ptr(a_out[2]));
   float *outs[3] = {ori, grad, coord};
   for (int q = 0; q < 3; q++) a.download(outs[q], a_out[q]);
   finish_stream(c);
   HS_API_END(c)
}

// k_assign_words on caller-supplied descriptors (hesaff_set_vocabulary: capi_impl.h)
int hesaff_stage_assign_words(hesaff_ctx *c, int n, const uint8_t *desc, int32_t *words_out)
{
   if (!c || n < 0 || (n > 0 && (!desc || !words_out))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   need_vocabulary(c);
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t N = (size_t)n;
   StageArena a(c);
   const Span<uint8_t> a_desc = a.add<uint8_t>(N * 128);
   const Span<int32_t> a_out = a.add<int32_t>(N * 2);   // (word, dist2) per key
   a.ensure();
   a.upload(a_desc, desc);
   launch_assign_words(c, a.ptr(a_desc), n, 128, 0, a.ptr(a_out));
   a.download(words_out, a_out);
   finish_stream(c);
   HS_API_END(c)
}

// k_assign_neighbours on caller-supplied descriptors (hesaff_set_vocabulary_neighbours: capi_impl.h): out[n][R][2], R the context's
int hesaff_stage_assign_neighbours(hesaff_ctx *c, int n, const uint8_t *desc, int32_t *neighbours_out)
{
   if (!c || n < 0 || (n > 0 && (!desc || !neighbours_out))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   need_vocabulary(c);
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t N = (size_t)n;
   StageArena a(c);
   const Span<uint8_t> a_desc = a.add<uint8_t>(N * 128);
   const Span<int32_t> a_out = a.add<int32_t>(N * 2 * (size_t)c->neighbours);   // (word, dist2) per key and rank
   a.ensure();
   a.upload(a_desc, desc);
   launch_assign_neighbours(c, a.ptr(a_desc), n, 128, 0, a.ptr(a_out));
   a.download(neighbours_out, a_out);
   finish_stream(c);
   HS_API_END(c)
}

} // extern "C"
