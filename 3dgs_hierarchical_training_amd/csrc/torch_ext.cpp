// torch_ext.cpp -- the PyTorch-ROCm extension over the C ABI of include/gsr.h (libgsr_hip.so).
//
// north_star: "Python host code calls HIP through a PyTorch-ROCm C++/HIP extension".  This file is that extension's host
// side: plain C++ (no kernels -- they live in *.hip behind the C ABI), built by torch.utils.cpp_extension into
// csrc/torch_build/gsr_torch.so and loaded with torch.ops.load_library.  It stands where the public module's
// `rasterize_points.cu / ext.cpp` pair stands (RasterizeGaussiansCUDA / RasterizeGaussiansBackwardCUDA / markVisible,
// called from diff_gaussian_rasterization/__init__.py as at /root/reference/scene/gaussian_model_ht.py:871-880):
//
//   gsr::rasterize            autograd-enabled entry (C++ torch::autograd::Function): what GaussianRasterizer.forward calls
//   gsr::rasterize_forward    -> gsr_forward   (buffers come from at::empty inside the allocator callback: no Python)
//   gsr::rasterize_backward   -> gsr_backward
//   gsr::rasterize_backward_frozen -> gsr_backward, the frozen call: camera / points_transform gradients alone
//   gsr::rasterize_backward_views  -> gsr_backward_views, that call over the output of rasterize_forward_views (V views of one model)
//   gsr::rasterize_backward_fused  -> gsr_backward with the in-kernel Adam step (parameters / moments updated in place)
//   gsr::render               -> gsr_forward, the render-only call: an image, nothing kept, no autograd
//   gsr::mark_visible         -> gsr_mark_visible
//   gsr::importance_accumulate -> gsr_forward + gsr_importance_accumulate (merge-time colour importance, no backward)
//   gsr::importance_pass      -> gsr_importance_accumulate over a rasterize_forward's outputs
//   gsr::photometric_loss_forward / _backward -> gsr_loss_forward / gsr_loss_backward
//   gsr::depth_loss_forward / _forward_stack / _backward, gsr::training_loss_terms -> gsr_depth_loss_forward / _backward / _forward_terms
//                                              and their _batched forms for stacks of planes
//   gsr::adam_step            -> gsr_adam_step
//   gsr::batch_retire         -> gsr_batch_retire (the per-model exit decision of a launch chain, written into the retire table)
//   gsr::retire_attach        attaches a retire table + step to the NEXT gsr::rasterize / render / importance_accumulate of the calling thread
//   gsr::pose_step            -> gsr_pose_step (stage A: tangent-space Adam + exponential map between two renders)
//   gsr::pose_step_many       -> gsr_pose_step_many (P such steps in one launch)
//   gsr::knn_mean_dist2       -> gsr_knn_mean_dist2
//   gsr::depth_to_points      -> gsr_depth_to_points (a depth map's pixels un-projected, colours gathered beside them)
//   gsr::voxel_down_sample    -> gsr_voxel_down_sample (voxel-grid means; its read of `meta` is the one host synchronisation)
//   gsr::camera_from_pose     -> gsr_camera_from_pose (view matrix, full projection and camera centre of up to 16 device poses, one launch)
//   gsr::pose_virtual_view    -> gsr_pose_virtual_view (the interpolated pose between two device poses, and that pose relative to a base)
//   gsr::resize_plan          -> gsr_resize_plan (flag bytes -> the source-row lists of the resized model; no host synchronisation)
//   gsr::resize_apply         -> gsr_resize_apply (every row of every parameter and moment tensor moved in one launch)
//   gsr::resize_plan_batched  -> gsr_resize_plan_batched (the same lists for every model of a batch; the launches do not depend on B)
//   gsr::resize_apply_batched -> gsr_resize_apply_batched (every row of the new store, padding included, in one launch)
//   gsr::select_smallest      -> gsr_select_smallest (the k rows with the smallest row maximum, as flag bytes; no host synchronisation)
//   gsr::merge_apply          -> gsr_merge_apply (the kept rows of two models appended in one launch)
//
// Registered with TORCH_LIBRARY so the ops are visible to the dispatcher (torch.ops.gsr.*, fake kernels in _ext.py for
// torch.compile).  An empty tensor (numel 0) stands for "None".  Everything runs on the current HIP stream of the
// inputs' device under a device guard.  No CPU kernels are registered: CPU tensors fail in the dispatcher.
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>   // a ROCm build of torch presents its HIP devices under the "cuda"
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>      // device type: these are its guard and stream accessors for them
#include <torch/library.h>
#include <torch/torch.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "../../include/gsr.h"

namespace {

using at::Tensor;

inline const float* fp(const Tensor& t) { return (t.defined() && t.numel() > 0) ? t.data_ptr<float>() : nullptr; }
inline float* fpm(Tensor& t) { return (t.defined() && t.numel() > 0) ? t.data_ptr<float>() : nullptr; }
inline bool has(const Tensor& t) { return t.defined() && t.numel() > 0; }

inline Tensor f32c(const Tensor& t)
{
    if (!has(t)) return t;
    return t.to(at::kFloat).contiguous();   // no-ops when already float32 + contiguous
}

void check(int rc, const char* what)
{
    TORCH_CHECK(rc == 0, what, " failed (code ", rc, "): ", gsr_last_error());
}

// GsrBatch from an op's `int[] batch_first_block` (B + 1 block offsets; fewer than three entries = a single model)
struct BatchArg {
    std::vector<int32_t> fb;
    GsrBatch b{};
    explicit BatchArg(at::IntArrayRef first_block)
    {
        if (first_block.size() >= 3) {
            fb.assign(first_block.begin(), first_block.end());
            b.B = (int32_t)fb.size() - 1;
            b.first_block = fb.data();
        }
    }
    const GsrBatch* ptr() const { return b.B > 1 ? &b : nullptr; }
    int64_t B() const { return b.B > 1 ? b.B : 1; }
};

struct AllocCtx {
    at::TensorOptions opts;
    Tensor binning;
    std::vector<Tensor> scratch;
};
void* alloc_cb(size_t bytes, int tag, void* user)
{
    AllocCtx* c = static_cast<AllocCtx*>(user);
    try {
        Tensor t = at::empty({(int64_t)bytes}, c->opts);
        if (tag == GSR_ALLOC_BINNING) c->binning = t;
        else c->scratch.push_back(t);
        return t.data_ptr();
    } catch (...) {
        return nullptr;   // out of memory -> GSR_ERR_ALLOC
    }
}

// diagnostics of the most recent forward of this process (bench.py reads R / R_eff from it, the binning test the list):
// {image workspace, binning, meta, [W, H]}
std::mutex g_last_mutex;
std::vector<Tensor> g_last;

std::vector<Tensor> debug_last()
{
    std::lock_guard<std::mutex> lk(g_last_mutex);
    return g_last;
}

// ---------------------------------------------------------------------------------------------------------------
// The retire table (gsr_forward_retire / GsrBackwardArgs::retired_at, version 117).  The schema strings of the existing ops stay as they are, so the table travels
// beside them: gsr::retire_attach(table, step) leaves it with the calling THREAD and the next forward-side op of that thread (rasterize /
// rasterize_forward, render, importance_accumulate) takes it -- single use.  gsr::rasterize keeps it with its autograd node, whose backward
// (another thread: autograd's device worker) attaches it again in front of the backward op it calls.  An empty tensor detaches.
struct RetirePending {
    Tensor table;
    int64_t step = 0;
};
thread_local RetirePending g_retire;

void retire_attach(const Tensor& retired_at, int64_t step)
{
    if (!has(retired_at)) { g_retire = RetirePending{}; return; }
    TORCH_CHECK(retired_at.is_cuda() && retired_at.scalar_type() == at::kInt && retired_at.is_contiguous() && retired_at.dim() == 1,
                "retire_attach: retired_at must be a contiguous int32 vector on the device (one entry per model)");
    g_retire.table = retired_at;
    g_retire.step = step;
}

RetirePending take_retire()
{
    RetirePending r = g_retire;
    g_retire = RetirePending{};
    return r;
}

// GsrForwardArgs::sh_origin as a contiguous float32 [3] tensor (undefined = none)
Tensor sh_origin_arg(const c10::optional<Tensor>& o)
{
    if (!o.has_value() || !o->defined()) return Tensor();
    TORCH_CHECK(o->numel() == 3 && o->is_cuda(), "sh_origin: three numbers on the device of the model expected");
    return f32c(o->reshape({3}));
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> rasterize_forward(
    const Tensor& means3D_, const Tensor& sh_, const Tensor& colors_, const Tensor& opacities_, const Tensor& scales_,
    const Tensor& rotations_, const Tensor& cov3D_, const Tensor& sh_rest_, const Tensor& viewmatrix_, const Tensor& projmatrix_,
    const Tensor& campos_, const Tensor& bg_, const Tensor& xf_, int64_t H, int64_t W, double tanfovx, double tanfovy,
    double scale_modifier, int64_t sh_degree, bool raw_params, bool prefiltered, bool debug, const Tensor& prepared,
    at::IntArrayRef batch_first_block, int64_t view_id, int64_t extras, const c10::optional<Tensor>& sh_origin_)
{
    const RetirePending retire = take_retire();
    TORCH_CHECK(means3D_.is_cuda(), "GaussianRasterizer: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const BatchArg batch(batch_first_block);
    const int64_t NB = batch.B();
    TORCH_CHECK(!retire.table.defined() || (retire.table.numel() == NB && retire.table.device() == means3D_.device()),
                "retired_at: one int32 entry per model of the batch, on the models' device");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D_.device());
    const Tensor means3D = f32c(means3D_), sh = f32c(sh_), colors = f32c(colors_), opac = f32c(opacities_), scales = f32c(scales_),
                 rots = f32c(rotations_), cov = f32c(cov3D_), rest = f32c(sh_rest_), vm = f32c(viewmatrix_), pm = f32c(projmatrix_),
                 campos = f32c(campos_), bg = f32c(bg_), xf = f32c(xf_);
    const Tensor sh_origin = sh_origin_arg(sh_origin_);
    const int64_t N = means3D.size(0);
    const int64_t M = has(sh) ? sh.size(1) + (has(rest) ? rest.size(1) : 0) : 0;
    const auto fo = means3D.options().dtype(at::kFloat);
    const auto bo = means3D.options().dtype(at::kByte);
    // batched render (GsrBatch): one image per model -- [B,3,H,W] / [B,1,H,W]; cameras are [B,4,4] / [B,3] / [B,3,4]
    if (NB > 1)
        TORCH_CHECK(vm.numel() == 16 * NB && pm.numel() == 16 * NB && (!has(campos) || campos.numel() == 3 * NB) && (!has(xf) || xf.numel() == 12 * NB),
                    "batch: viewmatrix / projmatrix must be [B,4,4], campos [B,3], points_transform [B,3,4]");
    Tensor color = NB > 1 ? at::empty({NB, 3, H, W}, fo) : at::empty({3, H, W}, fo);
    Tensor depth = NB > 1 ? at::empty({NB, 1, H, W}, fo) : at::empty({1, H, W}, fo);
    Tensor alpha = NB > 1 ? at::empty({NB, 1, H, W}, fo) : at::empty({1, H, W}, fo);
    // (prepared: the radii already sit in the hand-over buffer -- an int32 view of it, no copy)
    Tensor radii = has(prepared) ? prepared.slice(0, (int64_t)gsr_prepared_radii_offset((int32_t)N), (int64_t)gsr_prepared_radii_offset((int32_t)N) + 4 * N).view(at::kInt)
                                 : at::empty({N}, means3D.options().dtype(at::kInt));
    // "prepare in backward": the preceding backward already produced this render's splat records (+ keys, tile records) in
    // `prepared`; that buffer then IS the geometry workspace and the preprocess kernel is skipped
    if (has(prepared))
        TORCH_CHECK(prepared.is_contiguous() && prepared.scalar_type() == at::kByte &&
                        prepared.numel() == (int64_t)gsr_prepared_bytes((int32_t)N), "prepared buffer does not belong to this model");
    Tensor geom = has(prepared) ? prepared : at::empty({(int64_t)gsr_geom_bytes((int32_t)N)}, bo);
    Tensor image = at::empty({(int64_t)gsr_image_bytes_batched((int32_t)W, (int32_t)H, (int32_t)NB)}, bo);
    AllocCtx actx{bo, Tensor(), {}};

    GsrForwardArgs a{};
    a.N = (int32_t)N; a.M = (int32_t)M; a.D = (int32_t)sh_degree; a.W = (int32_t)W; a.H = (int32_t)H;
    a.prefiltered = prefiltered; a.debug = debug;
    a.scale_modifier = (float)scale_modifier; a.tanfovx = (float)tanfovx; a.tanfovy = (float)tanfovy;
    a.means3D = fp(means3D); a.scales = fp(scales); a.rotations = fp(rots); a.cov3D_precomp = fp(cov);
    a.opacities = fp(opac); a.shs = fp(sh); a.colors_precomp = fp(colors);
    a.viewmatrix = fp(vm); a.projmatrix = fp(pm); a.campos = fp(campos); a.bg = fp(bg);
    a.out_color = color.data_ptr<float>(); a.out_depth = depth.data_ptr<float>(); a.out_alpha = alpha.data_ptr<float>();
    a.radii = N ? radii.data_ptr<int32_t>() : nullptr;
    a.geom = geom.data_ptr(); a.image = image.data_ptr();
    a.alloc = alloc_cb; a.alloc_user = &actx;
    a.shs_rest = fp(rest); a.raw_params = raw_params;
    a.points_transform = fp(xf);
    a.prepared = has(prepared) ? prepared.data_ptr() : nullptr;
    a.batch = batch.ptr();
    a.view_id = view_id;
    a.sh_origin = fp(sh_origin);
    // extras: bit 0 = the clamped colour image (written by the blend kernel), bit 1 = the visibility bytes radii > 0 (written by the
    // preprocess; not available from a prepared buffer) -- what the reference's wrapper derives with one torch launch each
    Tensor clamped = (extras & 1) ? at::empty_like(color) : at::empty({0}, fo);
    Tensor visible = ((extras & 2) && !has(prepared)) ? at::empty({N}, bo) : at::empty({0}, bo);
    a.out_color_clamped = has(clamped) ? clamped.data_ptr<float>() : nullptr;
    a.visible = has(visible) ? visible.data_ptr<uint8_t>() : nullptr;
    GsrForwardOut out{};
    if (retire.table.defined())
        check(gsr_forward_retire(&a, retire.table.data_ptr<int32_t>(), retire.step, &out, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_forward_retire");
    else
        check(gsr_forward(&a, &out, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_forward");
    // (scratch tensors die here: stream-ordered reuse by the caching allocator is safe, same stream)
    Tensor meta = at::empty({3}, at::TensorOptions().dtype(at::kLong));   // CPU: R, capacity, flags
    int64_t* mp = meta.data_ptr<int64_t>();
    mp[0] = out.num_rendered; mp[1] = out.binning_capacity; mp[2] = out.forward_flags;
    Tensor binning = actx.binning.defined() ? actx.binning : at::empty({0}, bo);
    {
        Tensor dims = at::empty({3}, at::TensorOptions().dtype(at::kLong));
        dims.data_ptr<int64_t>()[0] = W; dims.data_ptr<int64_t>()[1] = H; dims.data_ptr<int64_t>()[2] = NB;
        std::lock_guard<std::mutex> lk(g_last_mutex);
        g_last = {image, binning, meta, dims};
    }
    return {color, radii, depth, alpha, geom, image, binning, meta, clamped, visible};
}

// gsr::importance_pass -> gsr_importance_accumulate over the outputs of a rasterize_forward of the same inputs on this stream (the second
// half of gsr::importance_accumulate below, on its own for callers that keep the forward's buffers).  Mutates acc only.
void importance_pass(Tensor& acc, const Tensor& means3D_, const Tensor& sh_, const Tensor& sh_rest_, const Tensor& campos_, const Tensor& xf_,
                     const Tensor& color, const Tensor& geom, const Tensor& image, const Tensor& binning, const Tensor& meta, int64_t H, int64_t W,
                     int64_t sh_degree, const c10::optional<Tensor>& sh_origin_)
{
    TORCH_CHECK(means3D_.is_cuda() && has(sh_), "importance_pass: a model with SH coefficients on a ROCm/HIP device expected");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D_.device());
    const Tensor means3D = f32c(means3D_), sh = f32c(sh_), rest = f32c(sh_rest_), campos = f32c(campos_), xf = f32c(xf_);
    const Tensor sh_origin = sh_origin_arg(sh_origin_);
    const int64_t N = means3D.size(0), M = sh.size(1) + (has(rest) ? rest.size(1) : 0);
    TORCH_CHECK(acc.is_cuda() && acc.scalar_type() == at::kFloat && acc.is_contiguous() && acc.dim() == 3 && acc.size(0) == N && acc.size(1) == M &&
                    acc.size(2) == 3, "importance: acc must be a contiguous float32 [N, M, 3] tensor (M = stored SH coefficients)");
    TORCH_CHECK(color.is_contiguous() && color.scalar_type() == at::kFloat && color.numel() == 3 * H * W && meta.numel() == 3 &&
                    geom.numel() == (int64_t)gsr_geom_bytes((int32_t)N) && image.numel() == (int64_t)gsr_image_bytes((int32_t)W, (int32_t)H),
                "importance_pass: the buffers do not come from a single-model rasterize_forward of this model and image size");
    GsrForwardArgs a{};
    a.N = (int32_t)N; a.M = (int32_t)M; a.D = (int32_t)sh_degree; a.W = (int32_t)W; a.H = (int32_t)H;
    a.means3D = fp(means3D); a.shs = fp(sh); a.shs_rest = fp(rest); a.campos = fp(campos); a.points_transform = fp(xf);
    a.sh_origin = fp(sh_origin);
    a.out_color = color.data_ptr<float>(); a.geom = geom.data_ptr(); a.image = image.data_ptr();
    GsrForwardOut out{};
    const int64_t* mp = meta.data_ptr<int64_t>();
    out.num_rendered = mp[0]; out.binning_capacity = mp[1]; out.forward_flags = mp[2];
    out.binning = has(binning) ? binning.data_ptr() : nullptr;
    if (out.binning) TORCH_CHECK(binning.numel() >= (int64_t)gsr_binning_bytes(mp[1] > 0 ? mp[1] : mp[0], (int32_t)W, (int32_t)H), "importance_pass: binning buffer too small");
    Tensor scratch = at::empty({(int64_t)gsr_importance_scratch_bytes((int32_t)N)}, means3D.options().dtype(at::kByte));
    check(gsr_importance_accumulate(&a, &out, acc.data_ptr<float>(), scratch.data_ptr(), c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()),
          "gsr_importance_accumulate");
}

// gsr::importance_accumulate -> gsr_forward + gsr_importance_accumulate: one view's colour importance added to `acc` [N,M,3] in place
// (include/gsr.h, version 113; what hierarchy.calc_importance's kernel route runs per view).  The render goes through rasterize_forward
// above -- the code path of gsr::rasterize -- with raw or activated parameters.  No autograd.  Returns the forward's
// {color, radii, depth, alpha, geom, image, binning, meta}: an ordinary rasterize_backward over them is still valid.
std::vector<Tensor> importance_accumulate(
    Tensor& acc, const Tensor& means3D_, const Tensor& sh_, const Tensor& colors_, const Tensor& opacities_, const Tensor& scales_,
    const Tensor& rotations_, const Tensor& cov3D_, const Tensor& sh_rest_, const Tensor& viewmatrix_, const Tensor& projmatrix_,
    const Tensor& campos_, const Tensor& bg_, const Tensor& xf_, int64_t H, int64_t W, double tanfovx, double tanfovy,
    double scale_modifier, int64_t sh_degree, bool raw_params, at::IntArrayRef batch_first_block, int64_t view_id,
    const c10::optional<Tensor>& sh_origin_)
{
    TORCH_CHECK(means3D_.is_cuda(), "importance_accumulate: tensors must be on a ROCm/HIP device (no CPU fallback)");
    // (gsr_importance_accumulate has no way to take a table -- include/gsr.h: refused here rather than ignored, before anything is enqueued)
    TORCH_CHECK(!take_retire().table.defined(), "importance_accumulate: a retire table (retired_at) is not served with the importance pass");
    const BatchArg batch(batch_first_block);
    TORCH_CHECK(batch.B() == 1, "importance_accumulate: not served with a batch of B > 1");
    TORCH_CHECK(has(sh_) && !has(colors_), "importance_accumulate: the model must carry SH coefficients (colors_precomp has none)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D_.device());
    const Tensor means3D = f32c(means3D_), sh = f32c(sh_), rest = f32c(sh_rest_), campos = f32c(campos_), xf = f32c(xf_);
    const int64_t N = means3D.size(0), M = sh.size(1) + (has(rest) ? rest.size(1) : 0);
    TORCH_CHECK(acc.is_cuda() && acc.scalar_type() == at::kFloat && acc.is_contiguous() && acc.dim() == 3 && acc.size(0) == N && acc.size(1) == M &&
                    acc.size(2) == 3, "importance_accumulate: acc must be a contiguous float32 [N, M, 3] tensor (M = stored SH coefficients)");
    auto f = rasterize_forward(means3D, sh, colors_, opacities_, scales_, rotations_, cov3D_, rest, viewmatrix_, projmatrix_, campos, bg_, xf, H, W,
                               tanfovx, tanfovy, scale_modifier, sh_degree, raw_params, false, false, at::empty({0}, means3D.options().dtype(at::kByte)),
                               batch_first_block, view_id, 0, sh_origin_);
    const Tensor &color = std::get<0>(f), &geom = std::get<4>(f), &image = std::get<5>(f), &binning = std::get<6>(f), &meta = std::get<7>(f);
    importance_pass(acc, means3D, sh, rest, campos, xf, color, geom, image, binning, meta, H, W, sh_degree, sh_origin_);
    return {color, std::get<1>(f), std::get<2>(f), std::get<3>(f), geom, image, binning, meta};
}

// gsr::rasterize_forward_views -> gsr_forward_views (include/gsr.h, version 123): ONE model under V cameras in one launch chain.
// viewmatrix / projmatrix are [V,4,4], campos [V,3], points_transform [V,3,4] and sh_origin [V,3] when given; V = viewmatrix.size(0).
// Returns {color [V,3,H,W], radii [V Npad], depth, alpha [V,1,H,W], geom, image, binning, meta, clamped, visible [V Npad]}; extras as in
// rasterize_forward.  No autograd key: rasterizer.rasterize_views pairs it with rasterize_backward_views (the frozen call over views).
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> rasterize_forward_views(
    const Tensor& means3D_, const Tensor& sh_, const Tensor& colors_, const Tensor& opacities_, const Tensor& scales_,
    const Tensor& rotations_, const Tensor& cov3D_, const Tensor& sh_rest_, const Tensor& viewmatrix_, const Tensor& projmatrix_,
    const Tensor& campos_, const Tensor& bg_, const Tensor& xf_, int64_t H, int64_t W, double tanfovx, double tanfovy,
    double scale_modifier, int64_t sh_degree, bool raw_params, int64_t extras, const c10::optional<Tensor>& sh_origin_)
{
    TORCH_CHECK(means3D_.is_cuda(), "rasterize_forward_views: tensors must be on a ROCm/HIP device (no CPU fallback)");
    TORCH_CHECK(!take_retire().table.defined(), "rasterize_forward_views: a retire table (retired_at) is not served with views");
    TORCH_CHECK(viewmatrix_.dim() == 3 && viewmatrix_.size(1) == 4 && viewmatrix_.size(2) == 4, "views: viewmatrix must be [V,4,4]");
    const int64_t V = viewmatrix_.size(0);
    TORCH_CHECK(V >= 1 && V <= GSR_MAX_VIEWS, "views: 1..16 views expected");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D_.device());
    const Tensor means3D = f32c(means3D_), sh = f32c(sh_), colors = f32c(colors_), opac = f32c(opacities_), scales = f32c(scales_),
                 rots = f32c(rotations_), cov = f32c(cov3D_), rest = f32c(sh_rest_), vm = f32c(viewmatrix_), pm = f32c(projmatrix_),
                 campos = f32c(campos_), bg = f32c(bg_), xf = f32c(xf_);
    Tensor sh_origin;
    if (sh_origin_.has_value() && sh_origin_->defined()) {
        TORCH_CHECK(sh_origin_->numel() == 3 * V && sh_origin_->is_cuda(), "views: sh_origin must be [V,3] on the device of the model");
        sh_origin = f32c(sh_origin_->reshape({V, 3}));
    }
    TORCH_CHECK(pm.numel() == 16 * V && (!has(campos) || campos.numel() == 3 * V) && (!has(xf) || xf.numel() == 12 * V),
                "views: projmatrix must be [V,4,4], campos [V,3], points_transform [V,3,4]");
    const int64_t N = means3D.size(0);
    TORCH_CHECK(N >= 1, "views: at least one Gaussian expected");
    const int64_t M = has(sh) ? sh.size(1) + (has(rest) ? rest.size(1) : 0) : 0;
    const int64_t Npad = (N + 127) / 128 * 128;
    TORCH_CHECK(V * Npad < ((int64_t)1 << 31), "views: V * Npad must stay below 2^31 records");
    const auto fo = means3D.options().dtype(at::kFloat);
    const auto bo = means3D.options().dtype(at::kByte);
    Tensor color = at::empty({V, 3, H, W}, fo), depth = at::empty({V, 1, H, W}, fo), alpha = at::empty({V, 1, H, W}, fo);
    Tensor radii = at::empty({V * Npad}, means3D.options().dtype(at::kInt));
    Tensor geom = at::empty({(int64_t)gsr_geom_bytes_views((int32_t)N, (int32_t)V)}, bo);
    Tensor image = at::empty({(int64_t)gsr_image_bytes_batched((int32_t)W, (int32_t)H, (int32_t)V)}, bo);
    AllocCtx actx{bo, Tensor(), {}};
    GsrForwardArgs a{};
    a.N = (int32_t)N; a.M = (int32_t)M; a.D = (int32_t)sh_degree; a.W = (int32_t)W; a.H = (int32_t)H;
    a.scale_modifier = (float)scale_modifier; a.tanfovx = (float)tanfovx; a.tanfovy = (float)tanfovy;
    a.means3D = fp(means3D); a.scales = fp(scales); a.rotations = fp(rots); a.cov3D_precomp = fp(cov);
    a.opacities = fp(opac); a.shs = fp(sh); a.colors_precomp = fp(colors);
    a.viewmatrix = fp(vm); a.projmatrix = fp(pm); a.campos = fp(campos); a.bg = fp(bg);
    a.out_color = color.data_ptr<float>(); a.out_depth = depth.data_ptr<float>(); a.out_alpha = alpha.data_ptr<float>();
    a.radii = radii.data_ptr<int32_t>();
    a.geom = geom.data_ptr(); a.image = image.data_ptr();
    a.alloc = alloc_cb; a.alloc_user = &actx;
    a.shs_rest = fp(rest); a.raw_params = raw_params;
    a.points_transform = fp(xf);
    a.sh_origin = fp(sh_origin);
    Tensor clamped = (extras & 1) ? at::empty_like(color) : at::empty({0}, fo);
    Tensor visible = (extras & 2) ? at::empty({V * Npad}, bo) : at::empty({0}, bo);
    a.out_color_clamped = has(clamped) ? clamped.data_ptr<float>() : nullptr;
    a.visible = has(visible) ? visible.data_ptr<uint8_t>() : nullptr;
    GsrForwardOut out{};
    check(gsr_forward_views(&a, (int32_t)V, &out, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_forward_views");
    Tensor meta = at::empty({3}, at::TensorOptions().dtype(at::kLong));   // CPU: R, capacity, flags
    int64_t* mp = meta.data_ptr<int64_t>();
    mp[0] = out.num_rendered; mp[1] = out.binning_capacity; mp[2] = out.forward_flags;
    Tensor binning = actx.binning.defined() ? actx.binning : at::empty({0}, bo);
    return {color, radii, depth, alpha, geom, image, binning, meta, clamped, visible};
}

// gsr::importance_accumulate_views -> gsr_forward_views + gsr_importance_accumulate_views: the colour importance of V views of one model
// added to `acc` [N,M,3] in place, view by view in the order given (what hierarchy.calc_importance runs per group of views).  Returns the
// forward's {color, radii, depth, alpha, geom, image, binning, meta}.
std::vector<Tensor> importance_accumulate_views(
    Tensor& acc, const Tensor& means3D_, const Tensor& sh_, const Tensor& colors_, const Tensor& opacities_, const Tensor& scales_,
    const Tensor& rotations_, const Tensor& cov3D_, const Tensor& sh_rest_, const Tensor& viewmatrix_, const Tensor& projmatrix_,
    const Tensor& campos_, const Tensor& bg_, const Tensor& xf_, int64_t H, int64_t W, double tanfovx, double tanfovy,
    double scale_modifier, int64_t sh_degree, bool raw_params, const c10::optional<Tensor>& sh_origin_)
{
    TORCH_CHECK(means3D_.is_cuda(), "importance_accumulate_views: tensors must be on a ROCm/HIP device (no CPU fallback)");
    TORCH_CHECK(has(sh_) && !has(colors_), "importance_accumulate_views: the model must carry SH coefficients (colors_precomp has none)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D_.device());
    const Tensor means3D = f32c(means3D_), sh = f32c(sh_), rest = f32c(sh_rest_), campos = f32c(campos_), xf = f32c(xf_);
    const int64_t N = means3D.size(0), M = sh.size(1) + (has(rest) ? rest.size(1) : 0);
    TORCH_CHECK(acc.is_cuda() && acc.scalar_type() == at::kFloat && acc.is_contiguous() && acc.dim() == 3 && acc.size(0) == N && acc.size(1) == M &&
                    acc.size(2) == 3, "importance_accumulate_views: acc must be a contiguous float32 [N, M, 3] tensor (M = stored SH coefficients)");
    auto f = rasterize_forward_views(means3D, sh, colors_, opacities_, scales_, rotations_, cov3D_, rest, viewmatrix_, projmatrix_, campos, bg_, xf, H, W,
                                     tanfovx, tanfovy, scale_modifier, sh_degree, raw_params, 0, sh_origin_);
    const Tensor &color = std::get<0>(f), &geom = std::get<4>(f), &image = std::get<5>(f), &binning = std::get<6>(f), &meta = std::get<7>(f);
    const int64_t V = color.size(0);
    Tensor sh_origin;
    if (sh_origin_.has_value() && sh_origin_->defined()) sh_origin = f32c(sh_origin_->reshape({V, 3}));
    GsrForwardArgs a{};
    a.N = (int32_t)N; a.M = (int32_t)M; a.D = (int32_t)sh_degree; a.W = (int32_t)W; a.H = (int32_t)H;
    a.means3D = fp(means3D); a.shs = fp(sh); a.shs_rest = fp(rest); a.campos = fp(campos); a.points_transform = fp(xf);
    a.sh_origin = fp(sh_origin);
    a.out_color = color.data_ptr<float>(); a.geom = geom.data_ptr(); a.image = image.data_ptr();
    GsrForwardOut out{};
    const int64_t* mp = meta.data_ptr<int64_t>();
    out.num_rendered = mp[0]; out.binning_capacity = mp[1]; out.forward_flags = mp[2];
    out.binning = has(binning) ? binning.data_ptr() : nullptr;
    Tensor scratch = at::empty({(int64_t)gsr_importance_scratch_bytes_views((int32_t)N, (int32_t)V)}, means3D.options().dtype(at::kByte));
    check(gsr_importance_accumulate_views(&a, (int32_t)V, &out, acc.data_ptr<float>(), scratch.data_ptr(),
                                          c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_importance_accumulate_views");
    return {color, std::get<1>(f), std::get<2>(f), std::get<3>(f), geom, image, binning, meta};
}

struct BwdCommon {
    Tensor means3D, sh, colors, opac, scales, rots, cov, rest, vm, pm, campos, bg, xf, gc, gd, ga;
};

void fill_backward_args(GsrBackwardArgs& a, const BwdCommon& b, const Tensor& geom, const Tensor& image, const Tensor& binning,
                        const Tensor& meta, int64_t H, int64_t W, double tanfovx, double tanfovy, double scale_modifier,
                        int64_t sh_degree, bool raw_params)
{
    const int64_t N = b.means3D.size(0);
    const int64_t M = has(b.sh) ? b.sh.size(1) + (has(b.rest) ? b.rest.size(1) : 0) : 0;
    const int64_t* mp = meta.data_ptr<int64_t>();
    a.N = (int32_t)N; a.M = (int32_t)M; a.D = (int32_t)sh_degree; a.W = (int32_t)W; a.H = (int32_t)H;
    a.scale_modifier = (float)scale_modifier; a.tanfovx = (float)tanfovx; a.tanfovy = (float)tanfovy;
    a.means3D = fp(b.means3D); a.scales = fp(b.scales); a.rotations = fp(b.rots); a.cov3D_precomp = fp(b.cov);
    a.opacities = fp(b.opac); a.shs = fp(b.sh); a.colors_precomp = fp(b.colors);
    a.viewmatrix = fp(b.vm); a.projmatrix = fp(b.pm); a.campos = fp(b.campos); a.bg = fp(b.bg);
    a.geom = geom.data_ptr(); a.image = image.data_ptr(); a.binning = has(binning) ? binning.data_ptr() : nullptr;
    a.num_rendered = mp[0]; a.binning_capacity = mp[1]; a.forward_flags = mp[2];
    a.grad_color = fp(b.gc); a.grad_depth = fp(b.gd); a.grad_alpha = fp(b.ga);
    a.shs_rest = fp(b.rest); a.raw_params = raw_params;
    a.points_transform = fp(b.xf);
}

// densification statistics accumulated by the backward kernel (GsrDensifyStats): stats = {xyz_gradient_accum, denom, max_radii2D}
// (N float32 elements each, updated in place), radii = the forward's int32 output.  Empty list = none.
bool fill_densify(GsrDensifyStats& ds, at::TensorList stats, const Tensor& radii, int64_t N)
{
    if (stats.empty()) return false;
    TORCH_CHECK(stats.size() == 3 && has(radii) && radii.scalar_type() == at::kInt && radii.numel() == N && radii.is_contiguous(),
                "densify_stats: three statistics tensors and the forward's radii expected");
    for (const Tensor& t : stats)
        TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() == N, "densify_stats: contiguous float32 tensors of N elements");
    ds.radii = radii.data_ptr<int32_t>();
    ds.xyz_gradient_accum = stats[0].data_ptr<float>(); ds.denom = stats[1].data_ptr<float>(); ds.max_radii2D = stats[2].data_ptr<float>();
    return true;
}

// returns {d_means3D, d_means2D, d_sh, d_colors, d_opac, d_scales, d_rot, d_cov, d_sh_rest, d_vm, d_pm, d_campos, d_xf}
std::vector<Tensor> rasterize_backward(
    const Tensor& means3D, const Tensor& sh, const Tensor& colors, const Tensor& opac, const Tensor& scales, const Tensor& rots,
    const Tensor& cov, const Tensor& rest, const Tensor& vm, const Tensor& pm, const Tensor& campos, const Tensor& bg, const Tensor& xf,
    const Tensor& geom, const Tensor& image, const Tensor& binning, const Tensor& meta, const Tensor& grad_color, const Tensor& grad_depth,
    const Tensor& grad_alpha, int64_t H, int64_t W, double tanfovx, double tanfovy, double scale_modifier, int64_t sh_degree,
    bool raw_params, bool need_vm, bool need_pm, bool need_campos, bool need_xf, at::TensorList densify_stats, const Tensor& radii,
    at::IntArrayRef batch_first_block, const c10::optional<Tensor>& sh_origin_)
{
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D.device());
    const BatchArg batch(batch_first_block);
    const int64_t NB = batch.B();
    BwdCommon b{means3D, sh, colors, opac, scales, rots, cov, rest, vm, pm, campos, bg, xf, f32c(grad_color), f32c(grad_depth), f32c(grad_alpha)};
    const int64_t N = means3D.size(0);
    const int64_t M = has(sh) ? sh.size(1) + (has(rest) ? rest.size(1) : 0) : 0;
    const auto fo = means3D.options().dtype(at::kFloat);
    Tensor none;
    Tensor d_means3D = at::empty({N, 3}, fo), d_means2D = at::empty({N, 3}, fo), d_opac = at::empty({N, 1}, fo);
    Tensor d_sh = has(sh) ? at::empty({N, has(rest) ? 1 : M, 3}, fo) : none;
    Tensor d_rest = (has(sh) && has(rest)) ? at::empty({N, M - 1, 3}, fo) : none;
    Tensor d_col = has(colors) ? at::empty({N, 3}, fo) : none;
    Tensor d_scales = has(scales) ? at::empty({N, 3}, fo) : none, d_rot = has(scales) ? at::empty({N, 4}, fo) : none;
    Tensor d_cov = has(cov) ? at::empty({N, 6}, fo) : none;
    auto cam_shape = [&](std::vector<int64_t> sh) { if (NB > 1) sh.insert(sh.begin(), NB); return sh; };
    Tensor d_vm = need_vm ? at::empty(cam_shape({4, 4}), fo) : none, d_pm = need_pm ? at::empty(cam_shape({4, 4}), fo) : none;
    Tensor d_cp = need_campos ? at::empty(cam_shape({3}), fo) : none;
    Tensor d_xf = (need_xf && has(xf)) ? at::zeros(cam_shape({3, 4}), fo) : none;
    Tensor scratch = at::empty({(int64_t)gsr_backward_scratch_bytes((int32_t)N)}, means3D.options().dtype(at::kByte));
    GsrBackwardArgs a{};
    fill_backward_args(a, b, geom, image, binning, meta, H, W, tanfovx, tanfovy, scale_modifier, sh_degree, raw_params);
    a.batch = batch.ptr();
    const Tensor sh_origin = sh_origin_arg(sh_origin_);
    a.sh_origin = fp(sh_origin);
    a.d_means3D = fpm(d_means3D); a.d_means2D = fpm(d_means2D); a.d_opacities = fpm(d_opac);
    a.d_colors_precomp = fpm(d_col); a.d_shs = fpm(d_sh); a.d_scales = fpm(d_scales); a.d_rotations = fpm(d_rot);
    a.d_cov3D_precomp = fpm(d_cov); a.d_shs_rest = fpm(d_rest);
    const RetirePending retire = take_retire();   // (refused by the library: a table needs the optimizer-in-backward)
    if (retire.table.defined()) { a.retired_at = retire.table.data_ptr<int32_t>(); a.retire_step = retire.step; }
    a.d_viewmatrix = fpm(d_vm); a.d_projmatrix = fpm(d_pm); a.d_campos = fpm(d_cp); a.d_points_transform = fpm(d_xf);
    a.scratch = scratch.data_ptr();
    GsrDensifyStats dstat{};
    if (fill_densify(dstat, densify_stats, radii, N)) a.densify_stats = &dstat;
    check(gsr_backward(&a, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_backward");
    return {d_means3D, d_means2D, d_sh, d_col, d_opac, d_scales, d_rot, d_cov, d_rest, d_vm, d_pm, d_cp, d_xf};
}

// The frozen call of gsr_backward (include/gsr.h, GsrBackwardArgs): the gradients of the camera and of points_transform alone -- no
// per-Gaussian gradient tensor is allocated, d_means2D only when somebody wants it.  Returns {d_means2D or undefined, d_vm, d_pm, d_campos, d_xf}.
std::vector<Tensor> rasterize_backward_frozen(
    const Tensor& means3D, const Tensor& sh, const Tensor& colors, const Tensor& opac, const Tensor& scales, const Tensor& rots,
    const Tensor& cov, const Tensor& rest, const Tensor& vm, const Tensor& pm, const Tensor& campos, const Tensor& bg, const Tensor& xf,
    const Tensor& geom, const Tensor& image, const Tensor& binning, const Tensor& meta, const Tensor& grad_color, const Tensor& grad_depth,
    const Tensor& grad_alpha, int64_t H, int64_t W, double tanfovx, double tanfovy, double scale_modifier, int64_t sh_degree,
    bool raw_params, bool need_means2D, bool need_vm, bool need_pm, bool need_campos, bool need_xf, at::IntArrayRef batch_first_block,
    const c10::optional<Tensor>& sh_origin_)
{
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D.device());
    const BatchArg batch(batch_first_block);
    const int64_t NB = batch.B();
    BwdCommon b{means3D, sh, colors, opac, scales, rots, cov, rest, vm, pm, campos, bg, xf, f32c(grad_color), f32c(grad_depth), f32c(grad_alpha)};
    const int64_t N = means3D.size(0);
    const auto fo = means3D.options().dtype(at::kFloat);
    Tensor none;
    Tensor d_means2D = need_means2D ? at::empty({N, 3}, fo) : none;
    auto cam_shape = [&](std::vector<int64_t> sh) { if (NB > 1) sh.insert(sh.begin(), NB); return sh; };
    Tensor d_vm = need_vm ? at::empty(cam_shape({4, 4}), fo) : none, d_pm = need_pm ? at::empty(cam_shape({4, 4}), fo) : none;
    Tensor d_cp = need_campos ? at::empty(cam_shape({3}), fo) : none;
    Tensor d_xf = (need_xf && has(xf)) ? at::zeros(cam_shape({3, 4}), fo) : none;
    TORCH_CHECK(d_vm.defined() || d_pm.defined() || d_cp.defined() || d_xf.defined(),
                "rasterize_backward_frozen: no camera or points_transform gradient is wanted -- nothing to compute");
    Tensor scratch = at::empty({(int64_t)gsr_backward_scratch_bytes((int32_t)N)}, means3D.options().dtype(at::kByte));
    GsrBackwardArgs a{};
    fill_backward_args(a, b, geom, image, binning, meta, H, W, tanfovx, tanfovy, scale_modifier, sh_degree, raw_params);
    a.batch = batch.ptr();
    const Tensor sh_origin = sh_origin_arg(sh_origin_);
    a.sh_origin = fp(sh_origin);
    a.d_means2D = fpm(d_means2D);
    a.d_viewmatrix = fpm(d_vm); a.d_projmatrix = fpm(d_pm); a.d_campos = fpm(d_cp); a.d_points_transform = fpm(d_xf);
    a.scratch = scratch.data_ptr();
    const RetirePending retire = take_retire();   // (refused by the library: no update to gate on the frozen backward)
    if (retire.table.defined()) { a.retired_at = retire.table.data_ptr<int32_t>(); a.retire_step = retire.step; }
    check(gsr_backward(&a, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_backward");
    return {d_means2D, d_vm, d_pm, d_cp, d_xf};
}

// gsr::rasterize_backward_views -> gsr_backward_views (include/gsr.h, version 124): the frozen call over the output of a
// rasterize_forward_views -- geom / image / binning / meta are that op's.  viewmatrix / projmatrix [V,4,4], campos [V,3], points_transform
// [V,3,4] and sh_origin [V,3] as in the forward; grad_color [V,3,H,W], grad_depth / grad_alpha [V,1,H,W] (or empty).  Returns
// {d_means2D [V Npad,3], d_viewmatrix [V,4,4], d_projmatrix [V,4,4], d_campos [V,3], d_points_transform [V,3,4]}, an empty tensor where
// the output is not wanted.  No autograd key: rasterizer.rasterize_views is the autograd node over the two ops.
std::vector<Tensor> rasterize_backward_views(
    const Tensor& means3D_, const Tensor& sh_, const Tensor& colors_, const Tensor& opac_, const Tensor& scales_, const Tensor& rots_,
    const Tensor& cov_, const Tensor& rest_, const Tensor& vm_, const Tensor& pm_, const Tensor& campos_, const Tensor& bg_, const Tensor& xf_,
    const Tensor& geom, const Tensor& image, const Tensor& binning, const Tensor& meta, const Tensor& grad_color, const Tensor& grad_depth,
    const Tensor& grad_alpha, int64_t H, int64_t W, double tanfovx, double tanfovy, double scale_modifier, int64_t sh_degree,
    bool raw_params, bool need_means2D, bool need_vm, bool need_pm, bool need_campos, bool need_xf, const c10::optional<Tensor>& sh_origin_)
{
    TORCH_CHECK(means3D_.is_cuda(), "rasterize_backward_views: tensors must be on a ROCm/HIP device (no CPU fallback)");
    TORCH_CHECK(!take_retire().table.defined(), "rasterize_backward_views: a retire table (retired_at) is not served with views");
    TORCH_CHECK(vm_.dim() == 3 && vm_.size(1) == 4 && vm_.size(2) == 4, "views: viewmatrix must be [V,4,4]");
    const int64_t V = vm_.size(0);
    TORCH_CHECK(V >= 1 && V <= GSR_MAX_VIEWS, "views: 1..16 views expected");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D_.device());
    BwdCommon b{f32c(means3D_), f32c(sh_), f32c(colors_), f32c(opac_), f32c(scales_), f32c(rots_), f32c(cov_), f32c(rest_), f32c(vm_), f32c(pm_),
                f32c(campos_), f32c(bg_), f32c(xf_), f32c(grad_color), f32c(grad_depth), f32c(grad_alpha)};
    Tensor sh_origin;
    if (sh_origin_.has_value() && sh_origin_->defined()) {
        TORCH_CHECK(sh_origin_->numel() == 3 * V && sh_origin_->is_cuda(), "views: sh_origin must be [V,3] on the device of the model");
        sh_origin = f32c(sh_origin_->reshape({V, 3}));
    }
    TORCH_CHECK(b.pm.numel() == 16 * V && (!has(b.campos) || b.campos.numel() == 3 * V) && (!has(b.xf) || b.xf.numel() == 12 * V),
                "views: projmatrix must be [V,4,4], campos [V,3], points_transform [V,3,4]");
    TORCH_CHECK((!has(b.gc) || b.gc.numel() == V * 3 * H * W) && (!has(b.gd) || b.gd.numel() == V * H * W) && (!has(b.ga) || b.ga.numel() == V * H * W),
                "views: grad_color must be [V,3,H,W], grad_depth and grad_alpha [V,1,H,W]");
    TORCH_CHECK(meta.defined() && !meta.is_cuda() && meta.scalar_type() == at::kLong && meta.numel() == 3, "views: meta must be the forward's");
    const int64_t N = b.means3D.size(0);
    TORCH_CHECK(N >= 1, "views: at least one Gaussian expected");
    const int64_t Npad = (N + 127) / 128 * 128;
    TORCH_CHECK(V * Npad < ((int64_t)1 << 31), "views: V * Npad must stay below 2^31 records");
    const auto fo = b.means3D.options().dtype(at::kFloat);
    const Tensor none = at::empty({0}, fo);
    const bool want_xf = need_xf && has(b.xf);
    TORCH_CHECK(need_vm || need_pm || need_campos || want_xf,
                "rasterize_backward_views: no camera or points_transform gradient is wanted -- nothing to compute");
    Tensor d_means2D = need_means2D ? at::empty({V * Npad, 3}, fo) : none;
    Tensor d_vm = need_vm ? at::empty({V, 4, 4}, fo) : none, d_pm = need_pm ? at::empty({V, 4, 4}, fo) : none;
    Tensor d_cp = need_campos ? at::empty({V, 3}, fo) : none;
    Tensor d_xf = want_xf ? at::zeros({V, 3, 4}, fo) : none;
    Tensor scratch = at::empty({(int64_t)gsr_backward_scratch_bytes_views((int32_t)N, (int32_t)V)}, b.means3D.options().dtype(at::kByte));
    GsrBackwardArgs a{};
    fill_backward_args(a, b, geom, image, binning, meta, H, W, tanfovx, tanfovy, scale_modifier, sh_degree, raw_params);
    a.sh_origin = fp(sh_origin);
    a.d_means2D = fpm(d_means2D);
    a.d_viewmatrix = fpm(d_vm); a.d_projmatrix = fpm(d_pm); a.d_campos = fpm(d_cp); a.d_points_transform = fpm(d_xf);
    a.scratch = scratch.data_ptr();
    check(gsr_backward_views(&a, (int32_t)V, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_backward_views");
    return {d_means2D, d_vm, d_pm, d_cp, d_xf};
}

// Optimizer-in-backward (GsrFusedAdam): parameters (xyz, f_dc, f_rest, opacity, scaling, rotation) and their moments are
// updated in place; returns {d_means2D, d_vm, d_pm, d_campos, d_xf}.
std::vector<Tensor> rasterize_backward_fused(
    Tensor means3D, Tensor sh, Tensor rest, Tensor opac, Tensor scales, Tensor rots, const Tensor& vm, const Tensor& pm, const Tensor& campos,
    const Tensor& bg, const Tensor& xf, const Tensor& geom, const Tensor& image, const Tensor& binning, const Tensor& meta,
    const Tensor& grad_color, const Tensor& grad_depth, const Tensor& grad_alpha, int64_t H, int64_t W, double tanfovx, double tanfovy,
    double scale_modifier, int64_t sh_degree, bool need_vm, bool need_pm, bool need_campos, bool need_xf, at::TensorList adam_m,
    at::TensorList adam_v, at::ArrayRef<double> adam_lr, double beta1, double beta2, double eps, int64_t step, const Tensor& next_vm,
    const Tensor& next_pm, const Tensor& next_campos, int64_t next_H, int64_t next_W, double next_tanfovx, double next_tanfovy,
    Tensor prepared_out, const Tensor& next_xf, int64_t next_sh_degree, at::TensorList densify_stats, const Tensor& radii,
    at::IntArrayRef batch_first_block, const c10::optional<Tensor>& sh_origin_)
{
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D.device());
    const BatchArg batch(batch_first_block);
    const int64_t NB = batch.B();
    // adam_lr: six learning rates, optionally followed by six step lags (GsrFusedAdam::step_lag; whole numbers)
    // deferred application (GsrFusedAdam::param_out): adam_m = six moments + six moment outputs + six parameter outputs, adam_v = six + six
    const bool deferred = adam_m.size() == 18 && adam_v.size() == 12;
    TORCH_CHECK(((adam_m.size() == 6 && adam_v.size() == 6) || deferred) && (adam_lr.size() == 6 || adam_lr.size() == 12), "fused_adam: six groups expected");
    Tensor none;
    BwdCommon b{means3D, sh, none, opac, scales, rots, none, rest, vm, pm, campos, bg, xf, f32c(grad_color), f32c(grad_depth), f32c(grad_alpha)};
    const int64_t N = means3D.size(0);
    const auto fo = means3D.options().dtype(at::kFloat);
    Tensor d_means2D = at::empty({N, 3}, fo);
    auto cam_shape = [&](std::vector<int64_t> sh) { if (NB > 1) sh.insert(sh.begin(), NB); return sh; };
    Tensor d_vm = need_vm ? at::empty(cam_shape({4, 4}), fo) : none, d_pm = need_pm ? at::empty(cam_shape({4, 4}), fo) : none;
    Tensor d_cp = need_campos ? at::empty(cam_shape({3}), fo) : none;
    Tensor d_xf = (need_xf && has(xf)) ? at::zeros(cam_shape({3, 4}), fo) : none;
    Tensor scratch = at::empty({(int64_t)gsr_backward_scratch_bytes((int32_t)N)}, means3D.options().dtype(at::kByte));
    GsrFusedAdam fa{};
    fa.beta1 = (float)beta1; fa.beta2 = (float)beta2; fa.eps = (float)eps; fa.step = step;
    for (int q = 0; q < 6; q++) {
        TORCH_CHECK(adam_m[q].is_contiguous() && adam_v[q].is_contiguous() && adam_m[q].scalar_type() == at::kFloat, "fused_adam: moments must be contiguous float32");
        fa.lr[q] = (float)adam_lr[q];
        fa.step_lag[q] = adam_lr.size() == 12 ? (int32_t)adam_lr[6 + q] : 0;
        fa.exp_avg[q] = adam_m[q].numel() ? adam_m[q].data_ptr<float>() : nullptr;     // (empty = the group is skipped: GsrFusedAdam)
        fa.exp_avg_sq[q] = adam_v[q].numel() ? adam_v[q].data_ptr<float>() : nullptr;
        if (deferred && adam_m[q].numel()) {
            TORCH_CHECK(adam_m[6 + q].is_contiguous() && adam_v[6 + q].is_contiguous() && adam_m[12 + q].is_contiguous() &&
                        adam_m[6 + q].numel() == adam_m[q].numel() && adam_v[6 + q].numel() == adam_m[q].numel() && adam_m[12 + q].numel() == adam_m[q].numel(),
                        "fused_adam (deferred): output buffers must be contiguous and shaped like their group");
            fa.exp_avg_out[q] = adam_m[6 + q].data_ptr<float>();
            fa.exp_avg_sq_out[q] = adam_v[6 + q].data_ptr<float>();
            fa.param_out[q] = adam_m[12 + q].data_ptr<float>();
        }
    }
    GsrBackwardArgs a{};
    fill_backward_args(a, b, geom, image, binning, meta, H, W, tanfovx, tanfovy, scale_modifier, sh_degree, true);
    a.d_means2D = fpm(d_means2D);
    a.d_viewmatrix = fpm(d_vm); a.d_projmatrix = fpm(d_pm); a.d_campos = fpm(d_cp); a.d_points_transform = fpm(d_xf);
    a.scratch = scratch.data_ptr();
    a.fused_adam = &fa;
    a.batch = batch.ptr();
    const RetirePending retire = take_retire();
    if (retire.table.defined()) {
        TORCH_CHECK(retire.table.numel() == NB, "retired_at: one int32 entry per model of the batch");
        a.retired_at = retire.table.data_ptr<int32_t>(); a.retire_step = retire.step;
    }
    const Tensor sh_origin = sh_origin_arg(sh_origin_);
    a.sh_origin = fp(sh_origin);
    GsrNextView nv{};
    // (the next render's own pose transform when its frame has one; otherwise it shares this render's)
    const Tensor nvm = f32c(next_vm), npm = f32c(next_pm), ncp = f32c(next_campos),
                 nxf = has(next_xf) ? f32c(NB > 1 ? next_xf : next_xf.slice(0, 0, 3)) : xf;
    if (has(prepared_out) && NB > 1)
        TORCH_CHECK(nvm.numel() == 16 * NB && npm.numel() == 16 * NB && ncp.numel() == 3 * NB, "batch: the next view's cameras must be [B,4,4] / [B,3]");
    if (has(prepared_out)) {   // "prepare in backward": this kernel also runs the NEXT render's preprocess on the updated parameters
        nv.W = (int32_t)next_W; nv.H = (int32_t)next_H; nv.D = (int32_t)(next_sh_degree >= 0 ? next_sh_degree : sh_degree);
        nv.scale_modifier = (float)scale_modifier; nv.tanfovx = (float)next_tanfovx; nv.tanfovy = (float)next_tanfovy;
        nv.viewmatrix = fp(nvm); nv.projmatrix = fp(npm); nv.campos = fp(ncp); nv.points_transform = fp(nxf);
        a.next_view = &nv;
        a.prepared_out = prepared_out.data_ptr();
    }
    GsrDensifyStats dstat{};
    if (fill_densify(dstat, densify_stats, radii, N)) a.densify_stats = &dstat;
    check(gsr_backward(&a, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_backward");
    return {d_means2D, d_vm, d_pm, d_cp, d_xf};
}

// ---------------------------------------------------------------------------------------------------------------
// autograd
// inputs (16 tensors): 0 means3D 1 means2D 2 sh 3 colors 4 opacities 5 scales 6 rotations 7 cov3D 8 sh_rest
//                      9 viewmatrix 10 projmatrix 11 campos 12 bg 13 points_transform
struct Cfg {
    int64_t H, W, sh_degree, adam_step;
    double tanfovx, tanfovy, scale_modifier, beta1, beta2, eps;
    bool raw_params, prefiltered, debug, cam_grad;
    std::vector<double> adam_lr;
    std::vector<Tensor> adam_m, adam_v;   // optimizer moments: plain buffers, not autograd inputs
    std::vector<int64_t> batch;           // first 128-Gaussian block of each model + the total (B + 1 entries), or empty: GsrBatch
    std::vector<Tensor> densify_stats;    // {xyz_gradient_accum, denom, max_radii2D} or empty: accumulated by the backward kernel
    Tensor adam_commit;                   // CPU int64 [1]: number of in-kernel Adam steps this optimizer's backwards have applied.  The
                                          // step count advances when a backward RUNS (a forward whose graph is dropped leaves no trace);
                                          // adam_step is the optimizer's step count at forward time, with adam_commit[0] as it was then
    Tensor prepared;                      // input: hand-over buffer of the preceding backward (or undefined)
    Tensor next_vm, next_pm, next_campos; // camera of the NEXT render (or undefined): the backward prepares it
    Tensor next_xf;                       // ... and its points_transform, when it differs from this render's (per-frame poses)
    int64_t next_H = 0, next_W = 0, next_D = -1;   // next_D: SH degree of the next render (-1 = this render's)
    int64_t view_id = 0;                           // GsrForwardArgs::view_id
    int64_t extras = 0;                            // bit 0: clamped colour output, bit 1: visibility bytes
    Tensor sh_origin;                              // GsrForwardArgs::sh_origin (detached, not an autograd input), or undefined
    int64_t frozen = -1;                           // the frozen backward (rasterize_backward_frozen): -1 = when no parameter wants a gradient, 0 = never, 1 = always
    double next_tanfovx = 0, next_tanfovy = 0;
};

class RasterizeFn : public torch::autograd::Function<RasterizeFn> {
   public:
    static torch::autograd::variable_list forward(torch::autograd::AutogradContext* ctx, const Tensor& means3D, const Tensor& means2D,
                                                  const Tensor& sh, const Tensor& colors, const Tensor& opac, const Tensor& scales,
                                                  const Tensor& rots, const Tensor& cov, const Tensor& rest, const Tensor& vm,
                                                  const Tensor& pm, const Tensor& campos, const Tensor& bg, const Tensor& xf,
                                                  const Cfg& cfg)
    {
        (void)means2D;
        static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::rasterize_forward", "").typed<decltype(rasterize_forward)>();
        // float32 + contiguous once, here: the SAME tensors are saved for the backward
        const Tensor m3 = f32c(means3D), s = f32c(sh), c = f32c(colors), o = f32c(opac), sc = f32c(scales), r = f32c(rots), cv = f32c(cov),
                     rs = f32c(rest), v = f32c(vm), p = f32c(pm), cp = f32c(campos), b = f32c(bg),
                     x = f32c((has(xf) && xf.dim() == 2) ? xf.slice(0, 0, 3) : xf);   // [4,4] -> rows 0..2; a batch hands [B,3,4]
        Tensor none;
        const RetirePending retire = g_retire;   // (peeked: rasterize_forward takes it; this node keeps it for its backward)
        ctx->saved_data["retire"] = retire.table.defined() ? retire.table : m3.new_empty({0}, m3.options().dtype(at::kInt));
        ctx->saved_data["retire_step"] = retire.step;
        auto out = op.call(m3, s, c, o, sc, r, cv, rs, v, p, cp, b, x, cfg.H, cfg.W, cfg.tanfovx, cfg.tanfovy, cfg.scale_modifier,
                           cfg.sh_degree, cfg.raw_params, cfg.prefiltered, cfg.debug, cfg.prepared.defined() ? cfg.prepared : x.new_empty({0}, x.options().dtype(at::kByte)),
                           cfg.batch, cfg.view_id, cfg.extras, cfg.sh_origin.defined() ? c10::optional<Tensor>(cfg.sh_origin) : c10::nullopt);
        // hand-over buffer for the NEXT render, filled by this render's backward (stream-ordered): allocated here so that it
        // can be returned to the caller as an ordinary output
        Tensor prep_out = has(cfg.next_vm) ? at::empty({(int64_t)gsr_prepared_bytes((int32_t)m3.size(0))}, m3.options().dtype(at::kByte))
                                           : at::empty({0}, m3.options().dtype(at::kByte));
        // NOTE: depth is deliberately NOT saved -- the caller mutates it in place (ht3dgs_trainer.py:1290-1292)
        std::vector<Tensor> saved = {m3, s, c, o, sc, r, cv, rs, v, p, cp, b, x, std::get<4>(out), std::get<5>(out), std::get<6>(out),
                                     std::get<7>(out)};
        const Tensor clamped = std::get<8>(out), visible = std::get<9>(out);
        if (has(clamped)) saved.push_back(std::get<0>(out));   // the raw colour: where it lies in [0, 1] a gradient on the clamped image passes
        ctx->saved_data["has_clamped"] = has(clamped);
        ctx->save_for_backward(saved);
        ctx->saved_data["adam_m"] = cfg.adam_m; ctx->saved_data["adam_v"] = cfg.adam_v;
        ctx->saved_data["dens"] = cfg.densify_stats;
        ctx->saved_data["batch"] = cfg.batch;
        ctx->saved_data["radii"] = cfg.densify_stats.empty() ? Tensor(at::empty({0}, m3.options().dtype(at::kInt))) : std::get<1>(out);
        ctx->saved_data["H"] = cfg.H; ctx->saved_data["W"] = cfg.W; ctx->saved_data["D"] = cfg.sh_degree;
        ctx->saved_data["tfx"] = cfg.tanfovx; ctx->saved_data["tfy"] = cfg.tanfovy; ctx->saved_data["smod"] = cfg.scale_modifier;
        ctx->saved_data["raw"] = cfg.raw_params; ctx->saved_data["cam_grad"] = cfg.cam_grad;
        ctx->saved_data["n_adam"] = (int64_t)cfg.adam_m.size();
        ctx->saved_data["lr"] = cfg.adam_lr; ctx->saved_data["b1"] = cfg.beta1; ctx->saved_data["b2"] = cfg.beta2;
        ctx->saved_data["eps"] = cfg.eps; ctx->saved_data["step"] = cfg.adam_step;
        ctx->saved_data["commit"] = cfg.adam_commit.defined() ? cfg.adam_commit : at::zeros({1}, at::TensorOptions().dtype(at::kLong));
        ctx->saved_data["commit_seen"] = cfg.adam_commit.defined() ? cfg.adam_commit.data_ptr<int64_t>()[0] : (int64_t)0;
        ctx->saved_data["xf_rows"] = (has(xf) && xf.dim() == 2) ? xf.size(0) : (int64_t)0;
        ctx->saved_data["done"] = false;
        ctx->saved_data["prep_out"] = prep_out;
        ctx->saved_data["sh_origin"] = cfg.sh_origin.defined() ? cfg.sh_origin : x.new_empty({0});
        ctx->saved_data["frozen"] = cfg.frozen;
        ctx->saved_data["next_cam"] = std::vector<Tensor>{has(cfg.next_vm) ? f32c(cfg.next_vm) : x, has(cfg.next_vm) ? f32c(cfg.next_pm) : x,
                                                          has(cfg.next_vm) ? f32c(cfg.next_campos) : x,
                                                          has(cfg.next_xf) ? f32c(cfg.next_xf) : x.new_empty({0})};
        ctx->saved_data["next_H"] = cfg.next_H; ctx->saved_data["next_W"] = cfg.next_W;
        ctx->saved_data["next_tfx"] = cfg.next_tanfovx; ctx->saved_data["next_tfy"] = cfg.next_tanfovy;
        ctx->saved_data["next_D"] = cfg.next_D;
        ctx->mark_non_differentiable({std::get<1>(out), prep_out, visible});
        ctx->set_materialize_grads(false);   // unused depth / alpha outputs arrive undefined -> specialised backward
        return {std::get<0>(out), std::get<1>(out), std::get<2>(out), std::get<3>(out), prep_out, clamped, visible};
    }

    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list g)
    {
        auto sv = ctx->get_saved_variables();
        const int64_t n_adam = ctx->saved_data["n_adam"].toInt();
        Tensor gc = g[0];
        const Tensor &gd = g[2], &ga = g[3];
        torch::autograd::variable_list out(15);   // 14 tensor inputs + the Cfg argument
        if (g.size() > 5 && g[5].defined() && ctx->saved_data["has_clamped"].toBool()) {
            // a gradient arrived on the CLAMPED image (a consumer that did not take the fused-clamp route): torch.clamp's rule
            const Tensor raw = sv.back();
            const Tensor pass = g[5] * raw.ge(0).logical_and(raw.le(1)).to(g[5].scalar_type());
            gc = gc.defined() ? gc + pass : pass;
        }
        if (!gc.defined() && !gd.defined() && !ga.defined()) return out;
        const int64_t H = ctx->saved_data["H"].toInt(), W = ctx->saved_data["W"].toInt(), D = ctx->saved_data["D"].toInt();
        const double tfx = ctx->saved_data["tfx"].toDouble(), tfy = ctx->saved_data["tfy"].toDouble(), smod = ctx->saved_data["smod"].toDouble();
        const bool raw = ctx->saved_data["raw"].toBool(), cam = ctx->saved_data["cam_grad"].toBool();
        const bool need_vm = cam && ctx->needs_input_grad(9), need_pm = cam && ctx->needs_input_grad(10), need_cp = cam && ctx->needs_input_grad(11);
        const bool need_xf = ctx->needs_input_grad(13);
        const int64_t xf_rows = ctx->saved_data["xf_rows"].toInt();
        Tensor e;
        auto orE = [&](const Tensor& t) { return t.defined() ? t : e; };
        Tensor d_xf;
        std::vector<Tensor> dens = ctx->saved_data["dens"].toTensorVector();
        const std::vector<int64_t> bfb = ctx->saved_data["batch"].toIntVector();
        const Tensor radii = ctx->saved_data["radii"].toTensor();
        const Tensor sho_t = ctx->saved_data["sh_origin"].toTensor();
        const c10::optional<Tensor> sho = has(sho_t) ? c10::optional<Tensor>(sho_t) : c10::nullopt;
        // the frozen backward: nobody reads a per-Gaussian gradient (inputs means3D, sh, colors, opacities, scales, rotations, cov3D, sh_rest)
        // and the camera or the transform wants one -- the pose phases of the reference, whose model does not move
        const int64_t frozen = ctx->saved_data["frozen"].toInt();
        const bool cam_wanted = need_vm || need_pm || need_cp || (need_xf && has(sv[12]));
        bool param_wanted = false;
        for (int q : {0, 2, 3, 4, 5, 6, 7, 8}) param_wanted = param_wanted || ctx->needs_input_grad(q);
        TORCH_CHECK(frozen != 1 || (!n_adam && dens.empty() && cam_wanted),
                    "frozen=True: not with fused_adam or densify_stats, and the camera or points_transform must require grad");
        const bool take_frozen = frozen == 1 || (frozen < 0 && !n_adam && dens.empty() && !param_wanted && cam_wanted);
        // the forward's retire table goes to whichever backward op runs below, on THIS thread (the op takes it; the library applies or refuses it)
        if (const Tensor rt = ctx->saved_data["retire"].toTensor(); has(rt)) retire_attach(rt, ctx->saved_data["retire_step"].toInt());
        if (n_adam) {
            // a second backward through the same forward would apply the optimizer step twice
            TORCH_CHECK(!ctx->saved_data["done"].toBool(), "fused_adam: backward() ran twice on the same render (retain_graph); the in-kernel "
                                                           "Adam step can be applied once per forward");
            ctx->saved_data["done"] = true;
            static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::rasterize_backward_fused", "").typed<decltype(rasterize_backward_fused)>();
            std::vector<Tensor> m = ctx->saved_data["adam_m"].toTensorVector(), v = ctx->saved_data["adam_v"].toTensorVector();
            auto lr = ctx->saved_data["lr"].toDoubleVector();
            auto nc = ctx->saved_data["next_cam"].toTensorVector();
            // the 1-based step of THIS update: the optimizer's count at forward time + the in-kernel steps applied since + 1
            Tensor commit = ctx->saved_data["commit"].toTensor();
            int64_t* commit_p = commit.data_ptr<int64_t>();
            const int64_t step_now = ctx->saved_data["step"].toInt() + (commit_p[0] - ctx->saved_data["commit_seen"].toInt()) + 1;
            auto r = op.call(sv[0], sv[1], sv[7], sv[3], sv[4], sv[5], sv[8], sv[9], sv[10], sv[11], sv[12], sv[13], sv[14], sv[15], sv[16],
                             orE(gc), orE(gd), orE(ga), H, W, tfx, tfy, smod, D, need_vm, need_pm, need_cp, need_xf, m, v, lr,
                             ctx->saved_data["b1"].toDouble(), ctx->saved_data["b2"].toDouble(), ctx->saved_data["eps"].toDouble(),
                             step_now, nc[0], nc[1], nc[2], ctx->saved_data["next_H"].toInt(),
                             ctx->saved_data["next_W"].toInt(), ctx->saved_data["next_tfx"].toDouble(), ctx->saved_data["next_tfy"].toDouble(),
                             ctx->saved_data["prep_out"].toTensor(), nc[3], ctx->saved_data["next_D"].toInt(), dens, radii, bfb, sho);
            commit_p[0] += 1;   // the update has been enqueued: the optimizer's step count advances (FusedAdam reconciles from this)
            out[1] = r[0]; out[9] = r[1]; out[10] = r[2]; out[11] = r[3]; d_xf = r[4];
        } else if (take_frozen) {
            static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::rasterize_backward_frozen", "").typed<decltype(rasterize_backward_frozen)>();
            auto r = op.call(sv[0], sv[1], sv[2], sv[3], sv[4], sv[5], sv[6], sv[7], sv[8], sv[9], sv[10], sv[11], sv[12], sv[13], sv[14],
                             sv[15], sv[16], orE(gc), orE(gd), orE(ga), H, W, tfx, tfy, smod, D, raw, ctx->needs_input_grad(1), need_vm, need_pm, need_cp,
                             need_xf, bfb, sho);
            out[1] = r[0]; out[9] = r[1]; out[10] = r[2]; out[11] = r[3]; d_xf = r[4];
        } else {
            static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::rasterize_backward", "").typed<decltype(rasterize_backward)>();
            auto r = op.call(sv[0], sv[1], sv[2], sv[3], sv[4], sv[5], sv[6], sv[7], sv[8], sv[9], sv[10], sv[11], sv[12], sv[13], sv[14],
                             sv[15], sv[16], orE(gc), orE(gd), orE(ga), H, W, tfx, tfy, smod, D, raw, need_vm, need_pm, need_cp, need_xf, dens, radii, bfb, sho);
            out[0] = r[0]; out[1] = r[1]; out[2] = r[2]; out[3] = r[3]; out[4] = r[4]; out[5] = r[5]; out[6] = r[6]; out[7] = r[7]; out[8] = r[8];
            out[9] = r[9]; out[10] = r[10]; out[11] = r[11]; d_xf = r[12];
        }
        if (d_xf.defined() && xf_rows == 4) d_xf = at::cat({d_xf, at::zeros({1, 4}, d_xf.options())}, 0);   // a [4,4] input keeps a zero last row
        out[13] = d_xf;
        return out;
    }
};

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> rasterize(
    const Tensor& means3D, const Tensor& means2D, const Tensor& sh, const Tensor& colors, const Tensor& opac, const Tensor& scales,
    const Tensor& rots, const Tensor& cov, const Tensor& rest, const Tensor& vm, const Tensor& pm, const Tensor& campos, const Tensor& bg,
    const Tensor& xf, int64_t H, int64_t W, double tanfovx, double tanfovy, double scale_modifier, int64_t sh_degree, bool raw_params,
    bool prefiltered, bool debug, bool cam_grad, at::TensorList adam_m, at::TensorList adam_v, at::ArrayRef<double> adam_lr, double beta1,
    double beta2, double eps, int64_t step, const Tensor& prepared, const Tensor& next_vm, const Tensor& next_pm, const Tensor& next_campos,
    int64_t next_H, int64_t next_W, double next_tanfovx, double next_tanfovy, const Tensor& next_xf, int64_t next_sh_degree,
    const Tensor& adam_commit, at::TensorList densify_stats, at::IntArrayRef batch_first_block, int64_t view_id, int64_t extras,
    const c10::optional<Tensor>& sh_origin, int64_t frozen)
{
    Cfg cfg{H, W, sh_degree, step, tanfovx, tanfovy, scale_modifier, beta1, beta2, eps, raw_params, prefiltered, debug, cam_grad,
            std::vector<double>(adam_lr.begin(), adam_lr.end()), adam_m.vec(), adam_v.vec()};
    if (has(prepared)) cfg.prepared = prepared;
    cfg.densify_stats = densify_stats.vec();
    cfg.batch.assign(batch_first_block.begin(), batch_first_block.end());
    cfg.view_id = view_id;
    cfg.extras = extras;
    cfg.frozen = frozen;
    if (sh_origin.has_value() && sh_origin->defined()) cfg.sh_origin = sh_origin->detach();
    if (!adam_m.empty()) {
        TORCH_CHECK(has(adam_commit) && adam_commit.is_cpu() && adam_commit.scalar_type() == at::kLong, "fused_adam: adam_commit must be a CPU int64 tensor");
        cfg.adam_commit = adam_commit;
    }
    if (has(next_vm)) {
        TORCH_CHECK(!adam_m.empty(), "prepare_next needs fused_adam (the backward that applies the update prepares the next render)");
        cfg.next_vm = next_vm; cfg.next_pm = next_pm; cfg.next_campos = next_campos;
        cfg.next_H = next_H; cfg.next_W = next_W; cfg.next_tanfovx = next_tanfovx; cfg.next_tanfovy = next_tanfovy;
        cfg.next_D = next_sh_degree;
        if (has(next_xf)) cfg.next_xf = next_xf;
    }
    auto r = RasterizeFn::apply(means3D, means2D, sh, colors, opac, scales, rots, cov, rest, vm, pm, campos, bg, xf, cfg);
    return {r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
}

// tensors without an autograd key (torch.inference_mode): the forward alone
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> rasterize_forward_only(
    const Tensor& means3D, const Tensor& means2D, const Tensor& sh, const Tensor& colors, const Tensor& opac, const Tensor& scales,
    const Tensor& rots, const Tensor& cov, const Tensor& rest, const Tensor& vm, const Tensor& pm, const Tensor& campos, const Tensor& bg,
    const Tensor& xf, int64_t H, int64_t W, double tanfovx, double tanfovy, double scale_modifier, int64_t sh_degree, bool raw_params,
    bool prefiltered, bool debug, bool cam_grad, at::TensorList adam_m, at::TensorList adam_v, at::ArrayRef<double> adam_lr, double beta1,
    double beta2, double eps, int64_t step, const Tensor& prepared, const Tensor& next_vm, const Tensor& next_pm, const Tensor& next_campos,
    int64_t next_H, int64_t next_W, double next_tanfovx, double next_tanfovy, const Tensor& next_xf, int64_t next_sh_degree,
    const Tensor& adam_commit, at::TensorList densify_stats, at::IntArrayRef batch_first_block, int64_t view_id, int64_t extras,
    const c10::optional<Tensor>& sh_origin, int64_t frozen)
{
    (void)frozen;
    (void)means2D; (void)next_xf; (void)next_sh_degree; (void)adam_commit; (void)densify_stats; (void)cam_grad; (void)adam_m; (void)adam_v; (void)adam_lr; (void)beta1; (void)beta2; (void)eps; (void)step;
    (void)next_vm; (void)next_pm; (void)next_campos; (void)next_H; (void)next_W; (void)next_tanfovx; (void)next_tanfovy;
    auto out = rasterize_forward(means3D, sh, colors, opac, scales, rots, cov, rest, vm, pm, campos, bg, (has(xf) && xf.dim() == 2) ? xf.slice(0, 0, 3) : xf, H, W,
                                 tanfovx, tanfovy, scale_modifier, sh_degree, raw_params, prefiltered, debug, prepared, batch_first_block, view_id, extras,
                                 sh_origin);
    return {std::get<0>(out), std::get<1>(out), std::get<2>(out), std::get<3>(out), at::empty({0}, means3D.options().dtype(at::kByte)), std::get<8>(out),
            std::get<9>(out)};
}

// gsr::render -> gsr_forward with GsrForwardArgs::render_only = 1 (include/gsr.h, version 116): the image of a model nobody will run a
// backward over -- a frozen teacher, an evaluation view.  No autograd registration and nothing saved: geom / image are NULL, so the
// library takes its splat records, its list and its counters as scratch that dies with this call, and what the allocator holds
// afterwards are the outputs.  outputs: bit 0 = depth + alpha, bit 1 = the clamped colour, bit 2 = the visibility bytes.
// Returns (color, radii, depth, alpha, clamped, visible), empty tensors for what was not asked.  g_last is left alone: last_call_info()
// and last_binning() keep describing the last FULL forward.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> render(
    const Tensor& means3D_, const Tensor& sh_, const Tensor& colors_, const Tensor& opacities_, const Tensor& scales_,
    const Tensor& rotations_, const Tensor& cov3D_, const Tensor& sh_rest_, const Tensor& viewmatrix_, const Tensor& projmatrix_,
    const Tensor& campos_, const Tensor& bg_, const Tensor& xf_, int64_t H, int64_t W, double tanfovx, double tanfovy,
    double scale_modifier, int64_t sh_degree, bool raw_params, int64_t view_id, int64_t outputs, const c10::optional<Tensor>& sh_origin_)
{
    const RetirePending retire = take_retire();   // (refused by the library: a render-only call takes no table)
    TORCH_CHECK(means3D_.is_cuda(), "render: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D_.device());
    const Tensor means3D = f32c(means3D_.detach()), sh = f32c(sh_.detach()), colors = f32c(colors_.detach()), opac = f32c(opacities_.detach()),
                 scales = f32c(scales_.detach()), rots = f32c(rotations_.detach()), cov = f32c(cov3D_.detach()), rest = f32c(sh_rest_.detach()),
                 vm = f32c(viewmatrix_.detach()), pm = f32c(projmatrix_.detach()), campos = f32c(campos_.detach()), bg = f32c(bg_.detach()),
                 xf = f32c(((has(xf_) && xf_.dim() == 2) ? xf_.slice(0, 0, 3) : xf_).detach());
    const Tensor sh_origin = sh_origin_arg(sh_origin_);
    const int64_t N = means3D.size(0);
    const int64_t M = has(sh) ? sh.size(1) + (has(rest) ? rest.size(1) : 0) : 0;
    const auto fo = means3D.options().dtype(at::kFloat);
    const auto bo = means3D.options().dtype(at::kByte);
    Tensor color = at::empty({3, H, W}, fo);
    Tensor depth = (outputs & 1) ? at::empty({1, H, W}, fo) : at::empty({0}, fo);
    Tensor alpha = (outputs & 1) ? at::empty({1, H, W}, fo) : at::empty({0}, fo);
    Tensor clamped = (outputs & 2) ? at::empty({3, H, W}, fo) : at::empty({0}, fo);
    Tensor visible = (outputs & 4) ? at::empty({N}, bo) : at::empty({0}, bo);
    Tensor radii = at::empty({N}, means3D.options().dtype(at::kInt));
    AllocCtx actx{bo, Tensor(), {}};

    GsrForwardArgs a{};
    a.N = (int32_t)N; a.M = (int32_t)M; a.D = (int32_t)sh_degree; a.W = (int32_t)W; a.H = (int32_t)H;
    a.scale_modifier = (float)scale_modifier; a.tanfovx = (float)tanfovx; a.tanfovy = (float)tanfovy;
    a.means3D = fp(means3D); a.scales = fp(scales); a.rotations = fp(rots); a.cov3D_precomp = fp(cov);
    a.opacities = fp(opac); a.shs = fp(sh); a.colors_precomp = fp(colors);
    a.viewmatrix = fp(vm); a.projmatrix = fp(pm); a.campos = fp(campos); a.bg = fp(bg);
    a.out_color = color.data_ptr<float>(); a.out_depth = fpm(depth); a.out_alpha = fpm(alpha);
    a.radii = N ? radii.data_ptr<int32_t>() : nullptr;
    a.alloc = alloc_cb; a.alloc_user = &actx;
    a.shs_rest = fp(rest); a.raw_params = raw_params;
    a.points_transform = fp(xf);
    a.view_id = view_id;
    a.sh_origin = fp(sh_origin);
    a.out_color_clamped = fpm(clamped);
    a.visible = has(visible) ? visible.data_ptr<uint8_t>() : nullptr;
    a.render_only = 1;
    GsrForwardOut out{};
    if (retire.table.defined())   // (refused: the library's own text)
        check(gsr_forward_retire(&a, retire.table.data_ptr<int32_t>(), retire.step, &out, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_forward_retire");
    else
        check(gsr_forward(&a, &out, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_forward");
    TORCH_CHECK(!actx.binning.defined() && out.binning == nullptr, "render: a render-only forward asked for a binning buffer");
    // (every scratch tensor dies here: stream-ordered reuse by the caching allocator is safe, same stream)
    return {color, radii, depth, alpha, clamped, visible};
}

// ---------------------------------------------------------------------------------------------------------------
Tensor mark_visible(const Tensor& means3D_, const Tensor& vm_, const Tensor& pm_)
{
    TORCH_CHECK(means3D_.is_cuda(), "markVisible: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D_.device());
    const Tensor p = f32c(means3D_), vm = f32c(vm_), pm = f32c(pm_);
    Tensor present = at::empty({p.size(0)}, p.options().dtype(at::kByte));
    check(gsr_mark_visible((int32_t)p.size(0), fp(p), fp(vm), fp(pm), p.size(0) ? present.data_ptr<uint8_t>() : nullptr,
                           c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_mark_visible");
    return present.to(at::kBool);
}

// render / target: [C,H,W], or a stack [B,C,H,W] of independent images (a batched render): then the loss is the SUM of the images'
// losses, each normalised by its own C H W, and every image receives the gradient of its own loss
std::tuple<Tensor, Tensor> photometric_loss_forward(const Tensor& render_, const Tensor& target_, double lambda_dssim, bool clamp)
{
    TORCH_CHECK(render_.is_cuda(), "fused_photometric_loss: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(render_.device());
    const Tensor render = f32c(render_), target = f32c(target_);
    TORCH_CHECK((render.dim() == 3 || render.dim() == 4) && render.sizes() == target.sizes(), "fused_photometric_loss: [C,H,W] or [B,C,H,W] render and target of one shape");
    const int o = render.dim() == 4 ? 1 : 0;
    const int32_t B = o ? (int32_t)render.size(0) : 1, C = (int32_t)render.size(o), H = (int32_t)render.size(o + 1), W = (int32_t)render.size(o + 2);
    Tensor ws = at::empty({(int64_t)gsr_loss_workspace_bytes_batched(B, C, H, W)}, render.options().dtype(at::kByte));
    Tensor out = at::empty({3}, render.options());
    check(gsr_loss_forward_batched(fp(render), fp(target), B, C, H, W, (float)lambda_dssim, clamp, ws.data_ptr(), out.data_ptr<float>(),
                                   c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_loss_forward");
    return {out, ws};
}

// the same with the six-term result vector of gsr_loss_forward_terms (single image)
std::tuple<Tensor, Tensor, Tensor> photometric_loss_forward_terms(const Tensor& render_, const Tensor& target_, double lambda_dssim, bool clamp)
{
    TORCH_CHECK(render_.is_cuda(), "fused_photometric_loss: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(render_.device());
    const Tensor render = f32c(render_), target = f32c(target_);
    TORCH_CHECK((render.dim() == 3 || render.dim() == 4) && render.sizes() == target.sizes(), "fused_photometric_loss: [C,H,W] or [B,C,H,W] render and target of one shape");
    const int o = render.dim() == 4 ? 1 : 0;
    const int32_t B = o ? (int32_t)render.size(0) : 1, C = (int32_t)render.size(o), H = (int32_t)render.size(o + 1), W = (int32_t)render.size(o + 2);
    Tensor ws = at::empty({(int64_t)gsr_loss_workspace_bytes_batched(B, C, H, W)}, render.options().dtype(at::kByte));
    Tensor out = at::empty({6}, render.options()), loss = at::empty({}, render.options());
    check(gsr_loss_forward_terms(fp(render), fp(target), B, C, H, W, (float)lambda_dssim, clamp, ws.data_ptr(), out.data_ptr<float>(),
                                 loss.data_ptr<float>(), c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_loss_forward_terms");
    return {out, ws, loss};
}

Tensor photometric_loss_backward(const Tensor& render_, const Tensor& target_, const Tensor& ws, const Tensor& grad_loss_, double lambda_dssim,
                                 bool clamp)
{
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(render_.device());
    const Tensor render = f32c(render_), target = f32c(target_), g = f32c(grad_loss_);
    const int o = render.dim() == 4 ? 1 : 0;
    const int32_t B = o ? (int32_t)render.size(0) : 1, C = (int32_t)render.size(o), H = (int32_t)render.size(o + 1), W = (int32_t)render.size(o + 2);
    Tensor d = at::empty_like(render);
    check(gsr_loss_backward_batched(fp(render), fp(target), B, C, H, W, (float)lambda_dssim, clamp, ws.data_ptr(), fp(g), d.data_ptr<float>(),
                                    c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_loss_backward");
    return d;
}

void adam_step(at::TensorList params, at::TensorList grads, at::TensorList exp_avg, at::TensorList exp_avg_sq, at::ArrayRef<double> lr,
               double beta1, double beta2, double eps, int64_t step)
{
    if (params.empty()) return;
    TORCH_CHECK(params[0].is_cuda(), "FusedAdam: parameters must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(params[0].device());
    std::vector<Tensor> keep;
    for (size_t lo = 0; lo < params.size(); lo += GSR_ADAM_MAX_TENSORS) {
        GsrAdamTensor arr[GSR_ADAM_MAX_TENSORS];
        const size_t n = std::min<size_t>(GSR_ADAM_MAX_TENSORS, params.size() - lo);
        for (size_t k = 0; k < n; k++) {
            const Tensor& p = params[lo + k];
            TORCH_CHECK(p.is_contiguous() && p.scalar_type() == at::kFloat, "FusedAdam: parameters must be contiguous float32");
            Tensor g = grads[lo + k].contiguous();
            keep.push_back(g);
            arr[k].param = p.data_ptr<float>(); arr[k].grad = g.data_ptr<float>();
            arr[k].exp_avg = exp_avg[lo + k].data_ptr<float>(); arr[k].exp_avg_sq = exp_avg_sq[lo + k].data_ptr<float>();
            arr[k].n = (uint64_t)p.numel(); arr[k].lr = (float)lr[lo + k];
        }
        check(gsr_adam_step(arr, (int32_t)n, (float)beta1, (float)beta2, (float)eps, step, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()),
              "gsr_adam_step");
    }
}

// The loss with its autograd node in C++ (one dispatcher call in the forward, no Python frame in the backward)
class PhotometricLossFn : public torch::autograd::Function<PhotometricLossFn> {
   public:
    static Tensor forward(torch::autograd::AutogradContext* ctx, const Tensor& render, const Tensor& target, double lambda_dssim, bool clamp)
    {
        static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::photometric_loss_forward", "").typed<decltype(photometric_loss_forward)>();
        const Tensor r = f32c(render), t = f32c(target.device() == render.device() ? target : target.to(render.device()));
        auto out = op.call(r, t, lambda_dssim, clamp);
        ctx->save_for_backward({r, t, std::get<1>(out)});
        ctx->saved_data["lam"] = lambda_dssim; ctx->saved_data["clamp"] = clamp;
        return std::get<0>(out).select(0, 0);
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list g)
    {
        static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::photometric_loss_backward", "").typed<decltype(photometric_loss_backward)>();
        auto sv = ctx->get_saved_variables();
        Tensor d = op.call(sv[0], sv[1], sv[2], g[0], ctx->saved_data["lam"].toDouble(), ctx->saved_data["clamp"].toBool());
        return {d, Tensor(), Tensor(), Tensor()};
    }
};
Tensor photometric_loss(const Tensor& render, const Tensor& target, double lambda_dssim, bool clamp)
{
    return PhotometricLossFn::apply(render, target, lambda_dssim, clamp);
}

// (loss, terms): `loss` is the differentiable scalar, `terms` the six-float vector {loss, mean SSIM, mean L1, loss_rgb, loss_dssim,
// loss_depth = 0} -- everything Loss.forward of the reference returns, from ONE forward; the caller slices it (views, no kernels).
// Undefined upstream gradients are not materialised: the backward sees d loss alone (no zero fills for the unused vector).
class PhotometricTermsFn : public torch::autograd::Function<PhotometricTermsFn> {
   public:
    static torch::autograd::variable_list forward(torch::autograd::AutogradContext* ctx, const Tensor& render, const Tensor& target, double lambda_dssim,
                                                  bool clamp)
    {
        const Tensor r = f32c(render), t = f32c(target.device() == render.device() ? target : target.to(render.device()));
        auto out = photometric_loss_forward_terms(r, t, lambda_dssim, clamp);
        ctx->save_for_backward({r, t, std::get<1>(out)});
        ctx->saved_data["lam"] = lambda_dssim; ctx->saved_data["clamp"] = clamp;
        Tensor terms = std::get<0>(out), loss = std::get<2>(out);   // (the scalar in storage of its own, written by the same kernel)
        ctx->mark_non_differentiable({terms});
        ctx->set_materialize_grads(false);
        return {loss, terms};
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list g)
    {
        if (!g[0].defined()) return {Tensor(), Tensor(), Tensor(), Tensor()};
        static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::photometric_loss_backward", "").typed<decltype(photometric_loss_backward)>();
        auto sv = ctx->get_saved_variables();
        Tensor d = op.call(sv[0], sv[1], sv[2], g[0], ctx->saved_data["lam"].toDouble(), ctx->saved_data["clamp"].toBool());
        return {d, Tensor(), Tensor(), Tensor()};
    }
};
std::tuple<Tensor, Tensor> photometric_loss_terms(const Tensor& render, const Tensor& target, double lambda_dssim, bool clamp)
{
    auto r = PhotometricTermsFn::apply(render, target, lambda_dssim, clamp);
    return {r[0], r[1]};
}
std::tuple<Tensor, Tensor> photometric_loss_terms_no_grad(const Tensor& render, const Tensor& target, double lambda_dssim, bool clamp)
{
    auto out = photometric_loss_forward_terms(render, target.device() == render.device() ? target : target.to(render.device()), lambda_dssim, clamp);
    return {std::get<2>(out), std::get<0>(out)};
}
Tensor photometric_loss_no_grad(const Tensor& render, const Tensor& target, double lambda_dssim, bool clamp)
{
    return std::get<0>(photometric_loss_forward(render, target.device() == render.device() ? target : target.to(render.device()), lambda_dssim, clamp)).select(0, 0);
}

// ---- the depth term of the loss (gsr_depth_loss_*): kind 0 = 'l1', 1 = 'invariant'.  depth / depth_gt are [H,W] or [1,H,W] planes, or
// stacks of B independent planes (gsr_depth_loss_*_batched): depth [B,1,H,W] (what a batched render returns) or [B,H,W] with B > 1,
// depth_gt [B,H,W] or [B,1,H,W] of the same B.  Returns the number of images of a stack, 0 for a plane.
static int32_t depth_dims(const Tensor& d, const Tensor& g, int32_t& H, int32_t& W)
{
    const bool plane = d.dim() == 2 || (d.dim() == 3 && d.size(0) == 1);
    const bool stack = (d.dim() == 3 && d.size(0) > 1) || (d.dim() == 4 && d.size(1) == 1);
    const bool gshape = !stack || ((g.dim() == 3 || (g.dim() == 4 && g.size(1) == 1)) && g.size(0) == d.size(0));
    TORCH_CHECK((plane || stack) && gshape && d.numel() > 0 && g.numel() == d.numel() && g.size(-1) == d.size(-1) && g.size(-2) == d.size(-2),
                "fused_depth_loss: [H,W] or [1,H,W] depth and depth_gt of one size, or stacks [B,1,H,W] / [B,H,W] of one B and one plane size");
    H = (int32_t)d.size(-2); W = (int32_t)d.size(-1);
    return stack ? (int32_t)d.size(0) : 0;
}
inline Tensor on_device_of(const Tensor& t, const Tensor& like) { return t.device() == like.device() ? t : t.to(like.device()); }

// {rows, workspace, sum}: a plane -> rows (6,), sum undefined (the plane's term is rows[0]); a stack -> rows [B,6], sum = the scalar
// SUM of the images' terms (written by the chain's last launch)
static std::tuple<Tensor, Tensor, Tensor> depth_loss_forward_any(const Tensor& depth_, const Tensor& gt_, int64_t kind, double clamp_lo, double clamp_hi)
{
    TORCH_CHECK(depth_.is_cuda(), "fused_depth_loss: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(depth_.device());
    const Tensor depth = f32c(depth_), gt = f32c(on_device_of(gt_, depth_));
    int32_t H, W;
    const int32_t B = depth_dims(depth, gt, H, W);
    if (B == 0) {
        Tensor ws = at::empty({(int64_t)gsr_depth_loss_workspace_bytes(H, W)}, depth.options().dtype(at::kByte));
        Tensor out = at::empty({6}, depth.options());
        check(gsr_depth_loss_forward(fp(depth), fp(gt), H, W, (int32_t)kind, (float)clamp_lo, (float)clamp_hi, 1.0f, ws.data_ptr(), out.data_ptr<float>(),
                                     c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_depth_loss_forward");
        return {out, ws, Tensor()};
    }
    Tensor ws = at::empty({(int64_t)gsr_depth_loss_workspace_bytes_batched(B, H, W)}, depth.options().dtype(at::kByte));
    Tensor out = at::empty({B, 6}, depth.options()), sum = at::empty({}, depth.options());
    check(gsr_depth_loss_forward_batched(fp(depth), fp(gt), B, H, W, (int32_t)kind, (float)clamp_lo, (float)clamp_hi, 1.0f, ws.data_ptr(),
                                         out.data_ptr<float>(), sum.data_ptr<float>(), c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()),
          "gsr_depth_loss_forward_batched");
    return {out, ws, sum};
}

// (rows, workspace): rows (6,) for a plane, the per-image rows [B,6] for a stack -- no gradient
std::tuple<Tensor, Tensor> depth_loss_forward(const Tensor& depth, const Tensor& gt, int64_t kind, double clamp_lo, double clamp_hi)
{
    auto out = depth_loss_forward_any(depth, gt, kind, clamp_lo, clamp_hi);
    return {std::get<0>(out), std::get<1>(out)};
}
// (sum, rows, workspace) of a stack: what the autograd nodes (DepthLossFn here, loss._FusedDepthLoss on the plain-FFI route) call
std::tuple<Tensor, Tensor, Tensor> depth_loss_forward_stack(const Tensor& depth, const Tensor& gt, int64_t kind, double clamp_lo, double clamp_hi)
{
    auto out = depth_loss_forward_any(depth, gt, kind, clamp_lo, clamp_hi);
    TORCH_CHECK(std::get<2>(out).defined(), "depth_loss_forward_stack: a stack [B,1,H,W] or [B,H,W] (a plane goes through depth_loss_forward)");
    return {std::get<2>(out), std::get<0>(out), std::get<1>(out)};
}

Tensor depth_loss_backward(const Tensor& depth_, const Tensor& gt_, const Tensor& ws, const Tensor& grad_loss_, int64_t kind, double clamp_lo,
                           double clamp_hi, double lambda_depth)
{
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(depth_.device());
    const Tensor depth = f32c(depth_), gt = f32c(on_device_of(gt_, depth_)), g = f32c(grad_loss_);
    int32_t H, W;
    const int32_t B = depth_dims(depth, gt, H, W);
    Tensor d = at::empty_like(depth);
    if (B == 0)
        check(gsr_depth_loss_backward(fp(depth), fp(gt), H, W, (int32_t)kind, (float)clamp_lo, (float)clamp_hi, (float)lambda_depth, ws.data_ptr(), fp(g),
                                      d.data_ptr<float>(), c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_depth_loss_backward");
    else {
        TORCH_CHECK(ws.numel() >= (int64_t)gsr_depth_loss_workspace_bytes_batched(B, H, W), "fused_depth_loss: the workspace of another stack");
        check(gsr_depth_loss_backward_batched(fp(depth), fp(gt), B, H, W, (int32_t)kind, (float)clamp_lo, (float)clamp_hi, (float)lambda_depth,
                                              ws.data_ptr(), fp(g), d.data_ptr<float>(), c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()),
              "gsr_depth_loss_backward_batched");
    }
    return d;
}

static bool depth_is_stack(const Tensor& d) { return (d.dim() == 3 && d.size(0) > 1) || d.dim() == 4; }

class DepthLossFn : public torch::autograd::Function<DepthLossFn> {
   public:
    static Tensor forward(torch::autograd::AutogradContext* ctx, const Tensor& depth, const Tensor& gt, int64_t kind, double lo, double hi)
    {
        static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::depth_loss_forward", "").typed<decltype(depth_loss_forward)>();
        static auto ops = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::depth_loss_forward_stack", "").typed<decltype(depth_loss_forward_stack)>();
        const Tensor d = f32c(depth), t = f32c(on_device_of(gt, depth));
        ctx->saved_data["kind"] = kind; ctx->saved_data["lo"] = lo; ctx->saved_data["hi"] = hi;
        if (depth_is_stack(d)) {      // the SUM of the images' terms
            auto out = ops.call(d, t, kind, lo, hi);
            ctx->save_for_backward({d, t, std::get<2>(out)});
            return std::get<0>(out);
        }
        auto out = op.call(d, t, kind, lo, hi);
        ctx->save_for_backward({d, t, std::get<1>(out)});
        return std::get<0>(out).select(0, 0);
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list g)
    {
        static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::depth_loss_backward", "").typed<decltype(depth_loss_backward)>();
        auto sv = ctx->get_saved_variables();
        Tensor d = op.call(sv[0], sv[1], sv[2], g[0], ctx->saved_data["kind"].toInt(), ctx->saved_data["lo"].toDouble(), ctx->saved_data["hi"].toDouble(), 1.0);
        return {d, Tensor(), Tensor(), Tensor(), Tensor()};
    }
};
Tensor depth_loss(const Tensor& depth, const Tensor& gt, int64_t kind, double lo, double hi) { return DepthLossFn::apply(depth, gt, kind, lo, hi); }
Tensor depth_loss_no_grad(const Tensor& depth, const Tensor& gt, int64_t kind, double lo, double hi)
{
    auto out = depth_loss_forward_any(depth, gt, kind, lo, hi);
    return std::get<2>(out).defined() ? std::get<2>(out) : std::get<0>(out).select(0, 0);
}

// The whole of Loss.forward (/root/reference/trainer/losses.py:98-136) with a depth term: (loss, terms), terms = {total loss, mean SSIM,
// mean L1, loss_rgb, loss_dssim, loss_depth (unweighted)} -- the photometric forward, then the depth chain whose last launch completes
// the vector.  ONE autograd node hands back d_render and d_depth.  A stack [B,3,H,W] with depth [B,1,H,W] / [B,H,W]: loss = the SUM of
// the images' losses (photometric and depth), terms[5] = the mean of the images' unweighted depth terms.
static std::tuple<Tensor, Tensor, Tensor, Tensor> training_loss_forward(const Tensor& r, const Tensor& t, const Tensor& dp, const Tensor& dg,
                                                                        double lambda_dssim, double lambda_depth, int64_t kind, bool clamp,
                                                                        double lo, double hi)
{
    auto out = photometric_loss_forward_terms(r, t, lambda_dssim, clamp);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(r.device());
    int32_t H, W;
    const int32_t B = depth_dims(dp, dg, H, W);
    TORCH_CHECK(r.dim() == 4 ? (B > 0 && r.size(0) == B) : B == 0,
                "fused_training_loss_report: a [C,H,W] render with a depth plane, or a [B,C,H,W] stack with a depth stack [B,1,H,W] / [B,H,W] of the same B");
    TORCH_CHECK(r.size(-2) == H && r.size(-1) == W, "fused_training_loss_report: render and depth of one image size");
    Tensor terms = std::get<0>(out), loss = std::get<2>(out);
    if (B == 0) {
        Tensor dws = at::empty({(int64_t)gsr_depth_loss_workspace_bytes(H, W)}, r.options().dtype(at::kByte)), dout = at::empty({6}, r.options());
        check(gsr_depth_loss_forward_terms(fp(dp), fp(dg), H, W, (int32_t)kind, (float)lo, (float)hi, (float)lambda_depth, dws.data_ptr(),
                                           dout.data_ptr<float>(), terms.data_ptr<float>(), loss.data_ptr<float>(),
                                           c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_depth_loss_forward_terms");
        return {loss, terms, std::get<1>(out), dws};
    }
    Tensor dws = at::empty({(int64_t)gsr_depth_loss_workspace_bytes_batched(B, H, W)}, r.options().dtype(at::kByte)), dout = at::empty({B, 6}, r.options());
    check(gsr_depth_loss_forward_terms_batched(fp(dp), fp(dg), B, H, W, (int32_t)kind, (float)lo, (float)hi, (float)lambda_depth, dws.data_ptr(),
                                               dout.data_ptr<float>(), terms.data_ptr<float>(), loss.data_ptr<float>(),
                                               c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_depth_loss_forward_terms_batched");
    return {loss, terms, std::get<1>(out), dws};
}
class TrainingLossFn : public torch::autograd::Function<TrainingLossFn> {
   public:
    static torch::autograd::variable_list forward(torch::autograd::AutogradContext* ctx, const Tensor& render, const Tensor& target, const Tensor& depth,
                                                  const Tensor& depth_gt, double lambda_dssim, double lambda_depth, int64_t kind, bool clamp, double lo,
                                                  double hi)
    {
        const Tensor r = f32c(render), t = f32c(on_device_of(target, render)), dp = f32c(depth), dg = f32c(on_device_of(depth_gt, render));
        auto out = training_loss_forward(r, t, dp, dg, lambda_dssim, lambda_depth, kind, clamp, lo, hi);
        ctx->save_for_backward({r, t, std::get<2>(out), dp, dg, std::get<3>(out)});
        ctx->saved_data["lam"] = lambda_dssim; ctx->saved_data["clamp"] = clamp; ctx->saved_data["lamd"] = lambda_depth;
        ctx->saved_data["kind"] = kind; ctx->saved_data["lo"] = lo; ctx->saved_data["hi"] = hi;
        Tensor loss = std::get<0>(out), terms = std::get<1>(out);
        ctx->mark_non_differentiable({terms});
        ctx->set_materialize_grads(false);
        return {loss, terms};
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list g)
    {
        torch::autograd::variable_list out(10);
        if (!g[0].defined()) return out;
        static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::photometric_loss_backward", "").typed<decltype(photometric_loss_backward)>();
        static auto opd = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::depth_loss_backward", "").typed<decltype(depth_loss_backward)>();
        auto sv = ctx->get_saved_variables();
        if (ctx->needs_input_grad(0)) out[0] = op.call(sv[0], sv[1], sv[2], g[0], ctx->saved_data["lam"].toDouble(), ctx->saved_data["clamp"].toBool());
        if (ctx->needs_input_grad(2))
            out[2] = opd.call(sv[3], sv[4], sv[5], g[0], ctx->saved_data["kind"].toInt(), ctx->saved_data["lo"].toDouble(), ctx->saved_data["hi"].toDouble(),
                              ctx->saved_data["lamd"].toDouble());
        return out;
    }
};
std::tuple<Tensor, Tensor> training_loss_terms(const Tensor& render, const Tensor& target, const Tensor& depth, const Tensor& depth_gt, double lambda_dssim,
                                               double lambda_depth, int64_t kind, bool clamp, double lo, double hi)
{
    auto r = TrainingLossFn::apply(render, target, depth, depth_gt, lambda_dssim, lambda_depth, kind, clamp, lo, hi);
    return {r[0], r[1]};
}
std::tuple<Tensor, Tensor> training_loss_terms_no_grad(const Tensor& render, const Tensor& target, const Tensor& depth, const Tensor& depth_gt,
                                                       double lambda_dssim, double lambda_depth, int64_t kind, bool clamp, double lo, double hi)
{
    auto out = training_loss_forward(f32c(render), f32c(on_device_of(target, render)), f32c(depth), f32c(on_device_of(depth_gt, render)), lambda_dssim,
                                     lambda_depth, kind, clamp, lo, hi);
    return {std::get<0>(out), std::get<1>(out)};
}

// Pose step of stage A: delta / exp_avg / exp_avg_sq ([6] float32) updated in place from dL/dM, the new M = Exp(delta) * base written
// into `xf` ([3,4] or [4,4] float32, rows 0..2) -- the tensor the next render reads as points_transform.  step = 0: only evaluates M.
void pose_step(Tensor delta, Tensor exp_avg, Tensor exp_avg_sq, const Tensor& d_xf, const Tensor& base, Tensor xf, double lr,
               double beta1, double beta2, double eps, int64_t step)
{
    TORCH_CHECK(delta.is_cuda(), "pose_step: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(delta.device());
    auto ok6 = [](const Tensor& t) { return t.is_contiguous() && t.scalar_type() == at::kFloat && t.numel() == 6; };
    TORCH_CHECK(ok6(delta) && (step == 0 || (ok6(exp_avg) && ok6(exp_avg_sq))), "pose_step: delta / moments must be contiguous float32 [6]");
    TORCH_CHECK(xf.is_contiguous() && xf.scalar_type() == at::kFloat && xf.numel() >= 12, "pose_step: xf must be contiguous float32 [3,4] or [4,4]");
    Tensor g = has(d_xf) ? f32c(d_xf) : d_xf, b = has(base) ? f32c(base) : base;
    TORCH_CHECK(step == 0 || (has(g) && g.numel() >= 12), "pose_step: d_xf must hold dL/dM (12 floats)");
    TORCH_CHECK(!has(b) || b.numel() >= 12, "pose_step: base must hold a 3x4 (or 4x4) matrix");
    check(gsr_pose_step(delta.data_ptr<float>(), step ? exp_avg.data_ptr<float>() : nullptr, step ? exp_avg_sq.data_ptr<float>() : nullptr,
                        fp(g), fp(b), xf.data_ptr<float>(), (float)lr, (float)beta1, (float)beta2, (float)eps, step,
                        c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_pose_step");
    // written through raw pointers: tell autograd's version counters (a hand-over buffer prepared for the old transform is then
    // recognised as stale, train_step._same_transform; a plain TORCH_LIBRARY op with a (a!) schema does not bump them itself)
    torch::autograd::impl::bump_version(xf);
    torch::autograd::impl::bump_version(delta);
}

// pose_step for P poses in ONE launch (gsr_pose_step_many): delta / exp_avg / exp_avg_sq [P,6], d_xf [P,3,4] (what rasterize_backward_views
// returns for points_transform), base [P,3,4] or empty (identity), xf [P,3,4] -- the tensor the next rasterize_forward_views reads.
void pose_step_many(Tensor delta, Tensor exp_avg, Tensor exp_avg_sq, const Tensor& d_xf, const Tensor& base, Tensor xf, double lr,
                    double beta1, double beta2, double eps, int64_t step)
{
    TORCH_CHECK(delta.is_cuda(), "pose_step_many: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(delta.device());
    TORCH_CHECK(delta.dim() == 2 && delta.size(1) == 6 && delta.size(0) >= 1, "pose_step_many: delta must be [P,6]");
    const int64_t P = delta.size(0);
    auto ok6 = [P](const Tensor& t) { return t.is_contiguous() && t.scalar_type() == at::kFloat && t.numel() == 6 * P; };
    TORCH_CHECK(ok6(delta) && (step == 0 || (ok6(exp_avg) && ok6(exp_avg_sq))), "pose_step_many: delta / moments must be contiguous float32 [P,6]");
    TORCH_CHECK(xf.is_contiguous() && xf.scalar_type() == at::kFloat && xf.numel() == 12 * P, "pose_step_many: xf must be contiguous float32 [P,3,4]");
    Tensor g = has(d_xf) ? f32c(d_xf) : d_xf, b = has(base) ? f32c(base) : base;
    TORCH_CHECK(step == 0 || (has(g) && g.numel() == 12 * P), "pose_step_many: d_xf must hold dL/dM of every pose ([P,3,4])");
    TORCH_CHECK(!has(b) || b.numel() == 12 * P, "pose_step_many: base must be [P,3,4]");
    check(gsr_pose_step_many(delta.data_ptr<float>(), step ? exp_avg.data_ptr<float>() : nullptr, step ? exp_avg_sq.data_ptr<float>() : nullptr,
                             fp(g), fp(b), xf.data_ptr<float>(), (int32_t)P, (float)lr, (float)beta1, (float)beta2, (float)eps, step,
                             c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_pose_step_many");
    torch::autograd::impl::bump_version(xf);   // (as pose_step)
    torch::autograd::impl::bump_version(delta);
}

// The pose matrix as an autograd node (round 6; what gsr_autopatch puts where the unmodified trainer evaluates `P[k].retr()`,
// /root/reference/scene/gaussian_model_ht.py:135-148): M = Exp(delta) * base as a [3,4] tensor from the pose's six tangent numbers,
// one one-wave kernel forward (gsr_pose_step with step 0), one backward (gsr_pose_grad: dL/dM -> dL/d(delta)); `delta` keeps its own
// shape ([6] or lietorch's [1,6]) and receives its .grad the usual way, so whichever optimizer owns it -- the FusedPoseAdam
// gsr_autopatch hands out, or a stock torch.optim.Adam -- steps it unchanged.  base: [3,4] / [4,4] or empty (identity).
Tensor pose_matrix_forward(const Tensor& delta, const Tensor& base)
{
    TORCH_CHECK(delta.is_cuda(), "pose_matrix: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(delta.device());
    TORCH_CHECK(delta.scalar_type() == at::kFloat && delta.numel() == 6, "pose_matrix: delta must hold six float32 numbers (tau, phi)");
    const Tensor d = delta.contiguous(), b = has(base) ? f32c(base) : base;
    TORCH_CHECK(!has(b) || b.numel() >= 12, "pose_matrix: base must hold a 3x4 (or 4x4) matrix");
    Tensor xf = at::empty({3, 4}, d.options());
    check(gsr_pose_step(const_cast<float*>(d.data_ptr<float>()), nullptr, nullptr, nullptr, fp(b), xf.data_ptr<float>(), 0.f, 0.9f, 0.999f, 1e-8f, 0,
                        c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_pose_step");
    return xf;
}
Tensor pose_matrix_backward(const Tensor& delta, const Tensor& base, const Tensor& d_xf)
{
    TORCH_CHECK(delta.is_cuda(), "pose_matrix: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(delta.device());
    const Tensor d = delta.contiguous(), b = has(base) ? f32c(base) : base, g = f32c(d_xf);
    TORCH_CHECK(d.scalar_type() == at::kFloat && d.numel() == 6 && g.numel() >= 12, "pose_matrix backward: delta [6], dL/dM [3,4]");
    Tensor out = at::empty(delta.sizes(), d.options());
    check(gsr_pose_grad(d.data_ptr<float>(), g.data_ptr<float>(), fp(b), out.data_ptr<float>(),
                        c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_pose_grad");
    return out;
}
class PoseMatrixFn : public torch::autograd::Function<PoseMatrixFn> {
   public:
    static Tensor forward(torch::autograd::AutogradContext* ctx, const Tensor& delta, const Tensor& base)
    {
        static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::pose_matrix_forward", "").typed<decltype(pose_matrix_forward)>();
        ctx->save_for_backward({delta, base});
        ctx->set_materialize_grads(false);
        return op.call(delta, base);
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list g)
    {
        if (!g[0].defined()) return {Tensor(), Tensor()};
        static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("gsr::pose_matrix_backward", "").typed<decltype(pose_matrix_backward)>();
        auto sv = ctx->get_saved_variables();
        return {op.call(sv[0], sv[1], g[0]), Tensor()};
    }
};
Tensor pose_matrix(const Tensor& delta, const Tensor& base) { return PoseMatrixFn::apply(delta, base); }

// Camera-route pose step: the frame's viewmatrix / projmatrix / campos tensors are rewritten in place from their own gradients.
void pose_step_camera(Tensor delta, Tensor exp_avg, Tensor exp_avg_sq, const Tensor& d_vm, const Tensor& d_pm, const Tensor& d_cp,
                      const Tensor& projT, const Tensor& base, Tensor vm, Tensor pm, Tensor cp, double lr, double beta1, double beta2,
                      double eps, int64_t step)
{
    TORCH_CHECK(delta.is_cuda(), "pose_step_camera: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(delta.device());
    auto okn = [](const Tensor& t, int64_t n) { return t.is_contiguous() && t.scalar_type() == at::kFloat && t.numel() == n; };
    TORCH_CHECK(okn(delta, 6) && (step == 0 || (okn(exp_avg, 6) && okn(exp_avg_sq, 6))), "pose_step_camera: delta / moments must be contiguous float32 [6]");
    TORCH_CHECK(okn(vm, 16) && okn(pm, 16) && okn(cp, 3), "pose_step_camera: viewmatrix / projmatrix [4,4] and campos [3] must be contiguous float32");
    const Tensor gv = has(d_vm) ? f32c(d_vm) : d_vm, gp = has(d_pm) ? f32c(d_pm) : d_pm, gc = has(d_cp) ? f32c(d_cp) : d_cp;
    const Tensor pt = f32c(projT), b = has(base) ? f32c(base) : base;
    TORCH_CHECK(pt.numel() == 16 && (!has(b) || b.numel() >= 12), "pose_step_camera: projection_T must be [4,4], base [3,4] or [4,4]");
    check(gsr_pose_step_camera(delta.data_ptr<float>(), step ? exp_avg.data_ptr<float>() : nullptr, step ? exp_avg_sq.data_ptr<float>() : nullptr,
                               fp(gv), fp(gp), fp(gc), fp(pt), fp(b), vm.data_ptr<float>(), pm.data_ptr<float>(), cp.data_ptr<float>(),
                               (float)lr, (float)beta1, (float)beta2, (float)eps, step,
                               c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_pose_step_camera");
    // (see pose_step: train_step._camera_versions compares these counters)
    torch::autograd::impl::bump_version(vm);
    torch::autograd::impl::bump_version(pm);
    torch::autograd::impl::bump_version(cp);
    torch::autograd::impl::bump_version(delta);
}

Tensor knn_mean_dist2(const Tensor& points_)
{
    TORCH_CHECK(points_.is_cuda(), "distCUDA2: points must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(points_.device());
    const Tensor p = f32c(points_);
    const int32_t N = (int32_t)p.size(0);
    Tensor out = at::empty({N}, p.options());
    const size_t sb = gsr_knn_scratch_bytes(N);
    Tensor scratch = at::empty({(int64_t)sb}, p.options().dtype(at::kByte));
    check(gsr_knn_mean_dist2(fp(p), N, N ? out.data_ptr<float>() : nullptr, scratch.data_ptr(), sb, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()),
          "gsr_knn_mean_dist2");
    return out;
}

// gsr::depth_to_points -> gsr_depth_to_points.  depth [H,W] (or [1,H,W] / [1,1,H,W]), image [3,H,W] or None -> (points [H*W,3],
// colors [H*W,3], or [0,3] without an image).  No autograd: inputs are detached.  No host synchronisation.
std::tuple<Tensor, Tensor> depth_to_points(const Tensor& depth_, const c10::optional<Tensor>& image_, double fx, double fy, double cx, double cy)
{
    TORCH_CHECK(depth_.is_cuda(), "depth_to_points: depth must be on a ROCm/HIP device (no CPU fallback)");
    TORCH_CHECK(depth_.dim() >= 2 && depth_.numel() == depth_.size(-2) * depth_.size(-1), "depth_to_points: depth is one plane [H,W]");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(depth_.device());
    const Tensor depth = f32c(depth_.detach());
    const int64_t H = depth.size(-2), W = depth.size(-1);
    TORCH_CHECK(H > 0 && W > 0 && H * W < ((int64_t)1 << 31), "depth_to_points: an image of 1 .. 2^31 - 1 pixels expected");
    const bool with_image = image_.has_value() && image_->defined();
    Tensor image;
    if (with_image) {
        TORCH_CHECK(image_->is_cuda() && image_->device() == depth_.device(), "depth_to_points: image must be on the depth's device (no CPU fallback)");
        TORCH_CHECK(image_->dim() == 3 && image_->size(0) == 3 && image_->size(1) == H && image_->size(2) == W, "depth_to_points: image is [3,H,W]");
        image = f32c(image_->detach());
    }
    Tensor points = at::empty({H * W, 3}, depth.options());
    Tensor colors = at::empty({with_image ? H * W : 0, 3}, depth.options());
    check(gsr_depth_to_points(depth.data_ptr<float>(), with_image ? image.data_ptr<float>() : nullptr, (int32_t)H, (int32_t)W, (float)fx, (float)fy,
                              (float)cx, (float)cy, points.data_ptr<float>(), with_image ? colors.data_ptr<float>() : nullptr,
                              c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_depth_to_points");
    return {points, colors};
}

// gsr::voxel_down_sample -> gsr_voxel_down_sample.  points [N,3], colors [N,3] or None -> (points [M,3], colors [M,3] or [0,3], counts [M] int32,
// dropped).  Scratch and the N-row outputs come from the allocator; the read of the four `meta` words is the one host synchronisation; the
// outputs are the first M rows of the N-row buffers.  status != 0 (an index beyond 2^21) raises.  No autograd: inputs are detached.
std::tuple<Tensor, Tensor, Tensor, int64_t> voxel_down_sample(const Tensor& points_, const c10::optional<Tensor>& colors_, double voxel_size)
{
    TORCH_CHECK(points_.is_cuda(), "voxel_down_sample: points must be on a ROCm/HIP device (no CPU fallback)");
    TORCH_CHECK(points_.dim() == 2 && points_.size(1) == 3, "voxel_down_sample: points is [N,3]");
    TORCH_CHECK(voxel_size > 0.0 && std::isfinite(voxel_size), "voxel_down_sample: voxel_size must be positive and finite");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(points_.device());
    const Tensor points = f32c(points_.detach());
    const int64_t N = points.size(0);
    TORCH_CHECK(N < ((int64_t)1 << 31), "voxel_down_sample: at most 2^31 - 1 points");
    const bool with_colors = colors_.has_value() && colors_->defined();
    Tensor colors;
    if (with_colors) {
        TORCH_CHECK(colors_->is_cuda() && colors_->device() == points_.device(), "voxel_down_sample: colors must be on the points' device (no CPU fallback)");
        TORCH_CHECK(colors_->dim() == 2 && colors_->size(0) == N && colors_->size(1) == 3, "voxel_down_sample: colors is [N,3]");
        colors = f32c(colors_->detach());
    }
    Tensor out_points = at::empty({N, 3}, points.options());
    Tensor out_colors = at::empty({with_colors ? N : 0, 3}, points.options());
    Tensor out_counts = at::empty({N}, points.options().dtype(at::kInt));
    Tensor meta = at::empty({4}, points.options().dtype(at::kLong));
    const size_t sb = gsr_voxel_scratch_bytes(N);
    Tensor scratch = at::empty({(int64_t)sb}, points.options().dtype(at::kByte));
    check(gsr_voxel_down_sample(N ? points.data_ptr<float>() : nullptr, (with_colors && N) ? colors.data_ptr<float>() : nullptr, N, voxel_size,
                                N ? out_points.data_ptr<float>() : nullptr, (with_colors && N) ? out_colors.data_ptr<float>() : nullptr,
                                N ? out_counts.data_ptr<int32_t>() : nullptr, meta.data_ptr<int64_t>(), N ? scratch.data_ptr() : nullptr, sb,
                                c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_voxel_down_sample");
    const Tensor host = meta.cpu();      // the feature's single host synchronisation
    const int64_t* h = host.data_ptr<int64_t>();
    TORCH_CHECK(h[2] == 0, "voxel_down_sample: extent / voxel_size needs a voxel index of 2^21 or more on some axis (status ", h[2],
                "): use a larger voxel_size or split the cloud");
    const int64_t M = h[0];
    return {out_points.narrow(0, 0, M), with_colors ? out_colors.narrow(0, 0, M) : out_colors, out_counts.narrow(0, 0, M), h[1]};
}

// gsr::camera_from_pose -> gsr_camera_from_pose.  pose [4,4] -> ([4,4], [4,4], [3]); pose [B,4,4] or [B,16] -> ([B,4,4], [B,4,4], [B,3]).
// No autograd: the pose is detached.  No host synchronisation.
std::tuple<Tensor, Tensor, Tensor> camera_from_pose(const Tensor& pose_, double fx, double fy, double cx, double cy, int64_t W, int64_t H,
                                                    double znear, double zfar)
{
    TORCH_CHECK(pose_.is_cuda(), "camera_from_pose: pose must be on a ROCm/HIP device (no CPU fallback)");
    const bool single = pose_.dim() == 2 && pose_.size(0) == 4 && pose_.size(1) == 4;
    TORCH_CHECK(single || (pose_.dim() == 3 && pose_.size(1) == 4 && pose_.size(2) == 4) || (pose_.dim() == 2 && pose_.size(1) == 16),
                "camera_from_pose: pose is [4,4], [B,4,4] or [B,16]");
    const int64_t B = single ? 1 : pose_.size(0);
    TORCH_CHECK(B >= 1 && B <= 16, "camera_from_pose: 1 to 16 poses per call, got ", B);
    TORCH_CHECK(fx > 0.0 && fy > 0.0 && W > 0 && H > 0 && W < ((int64_t)1 << 31) && H < ((int64_t)1 << 31),
                "camera_from_pose: fx, fy, W and H must be positive");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(pose_.device());
    const Tensor pose = f32c(pose_.detach());
    Tensor view = single ? at::empty({4, 4}, pose.options()) : at::empty({B, 4, 4}, pose.options());
    Tensor proj = at::empty_like(view);
    Tensor campos = single ? at::empty({3}, pose.options()) : at::empty({B, 3}, pose.options());
    check(gsr_camera_from_pose(pose.data_ptr<float>(), (int32_t)B, fx, fy, cx, cy, (int32_t)W, (int32_t)H, znear, zfar, view.data_ptr<float>(),
                               proj.data_ptr<float>(), campos.data_ptr<float>(), c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()),
          "gsr_camera_from_pose");
    return {view, proj, campos};
}

// gsr::pose_virtual_view -> gsr_pose_virtual_view.  pose0, pose1, base: [4,4] on one device; alpha in [0, 1].  Returns (out [4,4],
// out_rel [4,4], or an empty tensor without a base).  No autograd, no host synchronisation.
std::tuple<Tensor, Tensor> pose_virtual_view(const Tensor& pose0_, const Tensor& pose1_, double alpha, const c10::optional<Tensor>& base_)
{
    TORCH_CHECK(pose0_.is_cuda() && pose1_.is_cuda() && pose1_.device() == pose0_.device(),
                "pose_virtual_view: poses must be on one ROCm/HIP device (no CPU fallback)");
    TORCH_CHECK(pose0_.numel() == 16 && pose1_.numel() == 16, "pose_virtual_view: poses are [4,4]");
    TORCH_CHECK(alpha >= 0.0 && alpha <= 1.0, "pose_virtual_view: alpha must lie in [0, 1]");
    const bool with_base = base_.has_value() && base_->defined();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(pose0_.device());
    const Tensor p0 = f32c(pose0_.detach()), p1 = f32c(pose1_.detach());
    Tensor base;
    if (with_base) {
        TORCH_CHECK(base_->is_cuda() && base_->device() == pose0_.device() && base_->numel() == 16,
                    "pose_virtual_view: base is [4,4] on the poses' device (no CPU fallback)");
        base = f32c(base_->detach());
    }
    Tensor out = at::empty({4, 4}, p0.options());
    Tensor out_rel = with_base ? at::empty({4, 4}, p0.options()) : at::empty({0}, p0.options());
    check(gsr_pose_virtual_view(p0.data_ptr<float>(), p1.data_ptr<float>(), alpha, with_base ? base.data_ptr<float>() : nullptr,
                                out.data_ptr<float>(), with_base ? out_rel.data_ptr<float>() : nullptr,
                                c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_pose_virtual_view");
    return {out, out_rel};
}

// gsr::resize_plan -> gsr_resize_plan.  flags uint8 [N] -> (plan int32 [gsr_resize_plan_bytes(N) / 4], meta int64 [8], both on the device).
// No host synchronisation: the caller reads meta (its one wait) and hands the four counts to gsr::resize_apply.  No autograd.
std::tuple<Tensor, Tensor> resize_plan(const Tensor& flags_)
{
    TORCH_CHECK(flags_.is_cuda(), "resize_plan: flags must be on a ROCm/HIP device (no CPU fallback)");
    TORCH_CHECK(flags_.dim() == 1 && flags_.scalar_type() == at::kByte, "resize_plan: flags is uint8 [N]");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(flags_.device());
    const Tensor flags = flags_.contiguous();
    const int64_t N = flags.numel();
    const size_t pb = gsr_resize_plan_bytes(N), sb = gsr_resize_scratch_bytes(N);
    Tensor plan = at::empty({(int64_t)(pb / 4)}, flags.options().dtype(at::kInt));
    Tensor meta = at::empty({GSR_RESIZE_META_WORDS}, flags.options().dtype(at::kLong));
    Tensor scratch = at::empty({(int64_t)sb}, flags.options());
    check(gsr_resize_plan(N ? flags.data_ptr<uint8_t>() : nullptr, N, N ? plan.data_ptr() : nullptr, pb, meta.data_ptr<int64_t>(),
                          N ? scratch.data_ptr() : nullptr, sb, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_resize_plan");
    return {plan, meta};
}

// gsr::resize_apply -> gsr_resize_apply.  src[k]: [N, ...] contiguous, kinds[k]: GSR_RESIZE_PARAM / MOMENT / CHILD_SOURCED, child[k]: [2 nSplit, ...]
// for a CHILD_SOURCED tensor, an empty tensor otherwise.  Returns fresh tensors [nA + nB + 2 nC, ...].  check: read meta's status word back
// afterwards (a host synchronisation) and raise on a plan entry out of range; without it the call is asynchronous.  No autograd: surgery on
// detached storage.
std::vector<Tensor> resize_apply(const Tensor& plan, Tensor meta, int64_t N, int64_t nA, int64_t nB, int64_t nC, int64_t nSplit,
                                 at::TensorList src_, at::IntArrayRef kinds, at::TensorList child_, bool do_check)
{
    TORCH_CHECK(plan.is_cuda() && meta.is_cuda(), "resize_apply: plan and meta must be on a ROCm/HIP device (no CPU fallback)");
    TORCH_CHECK(plan.scalar_type() == at::kInt && plan.is_contiguous() && plan.dim() == 1, "resize_apply: plan is the int32 tensor of resize_plan");
    TORCH_CHECK(meta.scalar_type() == at::kLong && meta.is_contiguous() && meta.numel() == GSR_RESIZE_META_WORDS,
                "resize_apply: meta is the int64 [8] tensor of resize_plan");
    TORCH_CHECK(src_.size() == kinds.size() && src_.size() == child_.size(), "resize_apply: src, kinds and child have one entry per tensor");
    TORCH_CHECK((int64_t)src_.size() <= GSR_RESIZE_MAX_TENSORS, "resize_apply: at most ", GSR_RESIZE_MAX_TENSORS, " tensors");
    TORCH_CHECK(N >= 0 && nA >= 0 && nB >= 0 && nC >= 0 && nSplit >= 0, "resize_apply: negative count");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(plan.device());
    const int64_t nout = nA + nB + 2 * nC;
    std::vector<Tensor> src, child, dst;
    std::vector<GsrResizeTensor> table(src_.size());
    for (size_t k = 0; k < src_.size(); k++) {
        TORCH_CHECK(src_[k].is_cuda() && src_[k].device() == plan.device(), "resize_apply: src[", k, "] must be on the plan's device (no CPU fallback)");
        TORCH_CHECK(src_[k].dim() >= 1 && src_[k].size(0) == N, "resize_apply: src[", k, "] has N rows");
        src.push_back(src_[k].detach().contiguous());
        std::vector<int64_t> shape = src[k].sizes().vec();
        shape[0] = nout;
        dst.push_back(at::empty(shape, src[k].options()));
        int64_t row_bytes = (int64_t)src[k].element_size();
        for (size_t d = 1; d < shape.size(); d++) row_bytes *= shape[d];
        GsrResizeTensor& t = table[k];
        t.kind = (int32_t)kinds[k];
        t.row_bytes = row_bytes;
        const bool moves = row_bytes > 0 && nout > 0;
        t.src = (moves && N > 0) ? src[k].data_ptr() : nullptr;
        t.dst = (moves && N > 0) ? dst[k].data_ptr() : nullptr;
        t.child = nullptr;
        if (kinds[k] == GSR_RESIZE_CHILD_SOURCED && has(child_[k])) {
            TORCH_CHECK(child_[k].is_cuda() && child_[k].device() == plan.device(), "resize_apply: child[", k, "] must be on the plan's device (no CPU fallback)");
            TORCH_CHECK(child_[k].scalar_type() == src[k].scalar_type() && child_[k].size(0) == 2 * nSplit &&
                        child_[k].numel() * (int64_t)child_[k].element_size() == 2 * nSplit * row_bytes,
                        "resize_apply: child[", k, "] is [2 nSplit, ...] rows of its tensor");
            child.push_back(child_[k].detach().contiguous());
            t.child = child.back().data_ptr();
        }
    }
    check(gsr_resize_apply(plan.numel() ? plan.data_ptr() : nullptr, (size_t)plan.numel() * 4, N, nA, nB, nC, nSplit, table.data(), (int32_t)table.size(),
                           meta.data_ptr<int64_t>(), c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_resize_apply");
    if (do_check) {
        const Tensor host = meta.cpu();
        TORCH_CHECK(host.data_ptr<int64_t>()[GSR_RESIZE_META_STATUS] == 0, "resize_apply: the plan holds a row number outside [0, N) (status ",
                    host.data_ptr<int64_t>()[GSR_RESIZE_META_STATUS], "): the rows it names were written as zeros");
    }
    return dst;
}

static GsrResizeBatch resize_batch_of(const char* who, at::IntArrayRef first_block, at::IntArrayRef counts)
{
    TORCH_CHECK(counts.size() >= 1 && counts.size() <= GSR_RESIZE_MAX_MODELS, who, ": B must be in [1, ", GSR_RESIZE_MAX_MODELS, "]");
    TORCH_CHECK(first_block.size() == counts.size() + 1, who, ": first_block has B + 1 entries");
    GsrResizeBatch batch{};
    batch.B = (int32_t)counts.size();
    for (size_t b = 0; b < first_block.size(); b++) batch.first_block[b] = first_block[b];
    for (size_t b = 0; b < counts.size(); b++) batch.counts[b] = counts[b];
    return batch;
}

// gsr::resize_plan_batched -> gsr_resize_plan_batched.  flags uint8 [128 * first_block[B]] -> (plan int32, meta int64 [B, 8]); no host
// synchronisation, no autograd.
std::tuple<Tensor, Tensor> resize_plan_batched(const Tensor& flags_, at::IntArrayRef first_block, at::IntArrayRef counts)
{
    TORCH_CHECK(flags_.is_cuda(), "resize_plan_batched: flags must be on a ROCm/HIP device (no CPU fallback)");
    TORCH_CHECK(flags_.dim() == 1 && flags_.scalar_type() == at::kByte, "resize_plan_batched: flags is uint8 [N]");
    const GsrResizeBatch batch = resize_batch_of("resize_plan_batched", first_block, counts);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(flags_.device());
    const Tensor flags = flags_.contiguous();
    const int64_t N = flags.numel();
    TORCH_CHECK(N == GSR_RESIZE_BLOCK * first_block.back(), "resize_plan_batched: flags has 128 * first_block[B] entries");
    const size_t pb = gsr_resize_plan_bytes(N), sb = gsr_resize_scratch_bytes_batched(N);
    Tensor plan = at::empty({(int64_t)(pb / 4)}, flags.options().dtype(at::kInt));
    Tensor meta = at::empty({(int64_t)batch.B, GSR_RESIZE_META_WORDS}, flags.options().dtype(at::kLong));
    Tensor scratch = at::empty({(int64_t)sb}, flags.options());
    check(gsr_resize_plan_batched(N ? flags.data_ptr<uint8_t>() : nullptr, &batch, N ? plan.data_ptr() : nullptr, pb, meta.data_ptr<int64_t>(),
                                  N ? scratch.data_ptr() : nullptr, sb, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()),
          "gsr_resize_plan_batched");
    return {plan, meta};
}

// gsr::resize_apply_batched -> gsr_resize_apply_batched.  src[k]: [N, ...]; counts4: B x {nA, nB, nC, nSplit} flattened; child[k]: the models'
// children back to back ([2 sum nSplit_b, ...]) for a CHILD_SOURCED tensor, an empty tensor otherwise; pad[k]: one row of the tensor ([1, ...]
// or [...]) for the padding rows, an empty tensor for zeros.  Returns fresh tensors [128 * new_first_block[B], ...].  check as in resize_apply.
std::vector<Tensor> resize_apply_batched(const Tensor& plan, Tensor meta, at::IntArrayRef first_block, at::IntArrayRef counts, at::IntArrayRef counts4,
                                         at::IntArrayRef new_first_block, at::TensorList src_, at::IntArrayRef kinds, at::TensorList child_,
                                         at::TensorList pad_, bool do_check)
{
    TORCH_CHECK(plan.is_cuda() && meta.is_cuda(), "resize_apply_batched: plan and meta must be on a ROCm/HIP device (no CPU fallback)");
    TORCH_CHECK(plan.scalar_type() == at::kInt && plan.is_contiguous() && plan.dim() == 1, "resize_apply_batched: plan is the int32 tensor of resize_plan_batched");
    const GsrResizeBatch batch = resize_batch_of("resize_apply_batched", first_block, counts);
    const int64_t B = batch.B, N = GSR_RESIZE_BLOCK * first_block.back();
    TORCH_CHECK(meta.scalar_type() == at::kLong && meta.is_contiguous() && meta.numel() == B * GSR_RESIZE_META_WORDS,
                "resize_apply_batched: meta is the int64 [B, 8] tensor of resize_plan_batched");
    TORCH_CHECK((int64_t)counts4.size() == 4 * B && (int64_t)new_first_block.size() == B + 1,
                "resize_apply_batched: counts4 has 4 B entries and new_first_block B + 1");
    TORCH_CHECK(src_.size() == kinds.size() && src_.size() == child_.size() && src_.size() == pad_.size(),
                "resize_apply_batched: src, kinds, child and pad have one entry per tensor");
    TORCH_CHECK((int64_t)src_.size() <= GSR_RESIZE_MAX_TENSORS, "resize_apply_batched: at most ", GSR_RESIZE_MAX_TENSORS, " tensors");
    int64_t n_split = 0;
    for (int64_t b = 0; b < B; b++) {
        TORCH_CHECK(counts4[4 * b + 3] >= 0, "resize_apply_batched: negative count");
        n_split += counts4[4 * b + 3];
    }
    const int64_t nout = GSR_RESIZE_BLOCK * new_first_block.back();
    TORCH_CHECK(nout >= 0, "resize_apply_batched: negative new_first_block");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(plan.device());
    std::vector<Tensor> src, keep, dst;
    std::vector<GsrResizeBatchTensor> table(src_.size());
    for (size_t k = 0; k < src_.size(); k++) {
        TORCH_CHECK(src_[k].is_cuda() && src_[k].device() == plan.device(), "resize_apply_batched: src[", k, "] must be on the plan's device (no CPU fallback)");
        TORCH_CHECK(src_[k].dim() >= 1 && src_[k].size(0) == N, "resize_apply_batched: src[", k, "] has 128 * first_block[B] rows");
        src.push_back(src_[k].detach().contiguous());
        std::vector<int64_t> shape = src[k].sizes().vec();
        shape[0] = nout;
        dst.push_back(at::empty(shape, src[k].options()));
        int64_t row_bytes = (int64_t)src[k].element_size();
        for (size_t d = 1; d < shape.size(); d++) row_bytes *= shape[d];
        GsrResizeBatchTensor& t = table[k];
        t.kind = (int32_t)kinds[k];
        t.row_bytes = row_bytes;
        const bool moves = row_bytes > 0 && nout > 0 && N > 0;
        t.src = moves ? src[k].data_ptr() : nullptr;
        t.dst = moves ? dst[k].data_ptr() : nullptr;
        t.child = nullptr;
        t.pad = nullptr;
        if (kinds[k] == GSR_RESIZE_CHILD_SOURCED && has(child_[k])) {
            TORCH_CHECK(child_[k].is_cuda() && child_[k].device() == plan.device(), "resize_apply_batched: child[", k, "] must be on the plan's device (no CPU fallback)");
            TORCH_CHECK(child_[k].scalar_type() == src[k].scalar_type() && child_[k].size(0) == 2 * n_split &&
                        child_[k].numel() * (int64_t)child_[k].element_size() == 2 * n_split * row_bytes,
                        "resize_apply_batched: child[", k, "] is [2 sum nSplit_b, ...] rows of its tensor");
            keep.push_back(child_[k].detach().contiguous());
            t.child = keep.back().data_ptr();
        }
        if (has(pad_[k])) {
            TORCH_CHECK(pad_[k].is_cuda() && pad_[k].device() == plan.device(), "resize_apply_batched: pad[", k, "] must be on the plan's device (no CPU fallback)");
            TORCH_CHECK(pad_[k].scalar_type() == src[k].scalar_type() && pad_[k].numel() * (int64_t)pad_[k].element_size() == row_bytes,
                        "resize_apply_batched: pad[", k, "] is one row of its tensor");
            keep.push_back(pad_[k].detach().contiguous());
            t.pad = keep.back().data_ptr();
        }
    }
    check(gsr_resize_apply_batched(plan.numel() ? plan.data_ptr() : nullptr, (size_t)plan.numel() * 4, &batch, counts4.data(), new_first_block.data(),
                                   table.data(), (int32_t)table.size(), meta.data_ptr<int64_t>(),
                                   c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_resize_apply_batched");
    if (do_check) {
        const Tensor host = meta.cpu();
        for (int64_t b = 0; b < B; b++)
            TORCH_CHECK(host.data_ptr<int64_t>()[b * GSR_RESIZE_META_WORDS + GSR_RESIZE_META_STATUS] == 0, "resize_apply_batched: the plan holds a row "
                        "number outside model ", b, ": the rows it names were written as zeros");
    }
    return dst;
}

// gsr::select_smallest -> gsr_select_smallest.  values float32 [N, C] (or [N]: C = 1) -> (drop bool-as-uint8 [N], keep_flags uint8 [N],
// meta int64 [8]), all on the device.  No host synchronisation, no autograd.
std::tuple<Tensor, Tensor, Tensor> select_smallest(const Tensor& values_, int64_t k)
{
    TORCH_CHECK(values_.is_cuda(), "select_smallest: values must be on a ROCm/HIP device (no CPU fallback)");
    TORCH_CHECK((values_.dim() == 1 || values_.dim() == 2) && values_.scalar_type() == at::kFloat, "select_smallest: values is float32 [N, C] or [N]");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(values_.device());
    const Tensor values = values_.detach().contiguous();
    const int64_t N = values.size(0), C = values.dim() == 2 ? values.size(1) : 1;
    TORCH_CHECK(C >= 1 && C <= GSR_SELECT_MAX_COLUMNS, "select_smallest: C must be in [1, ", GSR_SELECT_MAX_COLUMNS, "]");
    const size_t sb = gsr_select_scratch_bytes(N);
    const auto bytes = values.options().dtype(at::kByte);
    Tensor drop = at::empty({N}, bytes), keep = at::empty({N}, bytes), scratch = at::empty({(int64_t)sb}, bytes);
    Tensor meta = at::empty({GSR_SELECT_META_WORDS}, values.options().dtype(at::kLong));
    check(gsr_select_smallest(N ? values.data_ptr<float>() : nullptr, N, (int32_t)C, k, drop.data_ptr<uint8_t>(), keep.data_ptr<uint8_t>(),
                              meta.data_ptr<int64_t>(), N ? scratch.data_ptr() : nullptr, sb,
                              c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_select_smallest");
    return {drop, keep, meta};
}

// gsr::merge_apply -> gsr_merge_apply.  src_a[k]: [Na, ...], src_b[k]: [Nb, ...] with the same trailing shape (an empty tensor for a MOMENT
// whose b rows do not exist), kinds[k]: GSR_RESIZE_PARAM / MOMENT.  Returns fresh tensors [nA + nB, ...].  check as in resize_apply.
std::vector<Tensor> merge_apply(const Tensor& plan_a, const Tensor& plan_b, Tensor meta, int64_t Na, int64_t nA, int64_t Nb, int64_t nB,
                                at::TensorList src_a_, at::TensorList src_b_, at::IntArrayRef kinds, bool do_check)
{
    TORCH_CHECK(plan_a.is_cuda() && plan_b.is_cuda() && meta.is_cuda(), "merge_apply: the plans and meta must be on a ROCm/HIP device (no CPU fallback)");
    TORCH_CHECK(plan_a.scalar_type() == at::kInt && plan_a.is_contiguous() && plan_a.dim() == 1 && plan_b.scalar_type() == at::kInt &&
                plan_b.is_contiguous() && plan_b.dim() == 1, "merge_apply: plan_a and plan_b are int32 tensors of resize_plan");
    TORCH_CHECK(meta.scalar_type() == at::kLong && meta.is_contiguous() && meta.numel() == GSR_RESIZE_META_WORDS,
                "merge_apply: meta is the int64 [8] tensor of resize_plan");
    TORCH_CHECK(src_a_.size() == kinds.size() && src_a_.size() == src_b_.size(), "merge_apply: src_a, src_b and kinds have one entry per tensor");
    TORCH_CHECK((int64_t)src_a_.size() <= GSR_RESIZE_MAX_TENSORS, "merge_apply: at most ", GSR_RESIZE_MAX_TENSORS, " tensors");
    TORCH_CHECK(Na >= 0 && nA >= 0 && Nb >= 0 && nB >= 0, "merge_apply: negative count");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(plan_a.device());
    const int64_t nout = nA + nB;
    std::vector<Tensor> src_a, src_b, dst;
    std::vector<GsrMergeTensor> table(src_a_.size());
    for (size_t k = 0; k < src_a_.size(); k++) {
        TORCH_CHECK(src_a_[k].is_cuda() && src_a_[k].device() == plan_a.device() && src_b_[k].is_cuda() && src_b_[k].device() == plan_a.device(),
                    "merge_apply: src_a[", k, "] and src_b[", k, "] must be on the plans' device (no CPU fallback)");
        TORCH_CHECK(src_a_[k].dim() >= 1 && src_a_[k].size(0) == Na, "merge_apply: src_a[", k, "] has Na rows");
        src_a.push_back(src_a_[k].detach().contiguous());
        std::vector<int64_t> shape = src_a[k].sizes().vec();
        int64_t row_bytes = (int64_t)src_a[k].element_size();
        for (size_t d = 1; d < shape.size(); d++) row_bytes *= shape[d];
        const bool absent_b = kinds[k] == GSR_RESIZE_MOMENT && src_b_[k].dim() == 1 && src_b_[k].numel() == 0;
        if (!absent_b) {
            shape[0] = Nb;
            TORCH_CHECK(src_b_[k].sizes().vec() == shape && src_b_[k].scalar_type() == src_a[k].scalar_type(),
                        "merge_apply: src_b[", k, "] is [Nb, ...] with src_a's trailing shape and dtype");
        }
        src_b.push_back(src_b_[k].detach().contiguous());
        shape[0] = nout;
        dst.push_back(at::empty(shape, src_a[k].options()));
        GsrMergeTensor& t = table[k];
        t.kind = (int32_t)kinds[k];
        t.row_bytes = row_bytes;
        t.reserved = 0;
        const bool moves = row_bytes > 0 && nout > 0;
        t.src_a = (moves && Na > 0) ? src_a[k].data_ptr() : nullptr;
        t.src_b = (moves && !absent_b && Nb > 0) ? src_b[k].data_ptr() : nullptr;
        t.dst = moves ? dst[k].data_ptr() : nullptr;
    }
    check(gsr_merge_apply(plan_a.numel() ? plan_a.data_ptr() : nullptr, (size_t)plan_a.numel() * 4, Na, nA, plan_b.numel() ? plan_b.data_ptr() : nullptr,
                          (size_t)plan_b.numel() * 4, Nb, nB, table.data(), (int32_t)table.size(), meta.data_ptr<int64_t>(),
                          c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_merge_apply");
    if (do_check) {
        const Tensor host = meta.cpu();
        TORCH_CHECK(host.data_ptr<int64_t>()[GSR_RESIZE_META_STATUS] == 0, "merge_apply: a plan holds a row number outside its model (status ",
                    host.data_ptr<int64_t>()[GSR_RESIZE_META_STATUS], "): the rows it names were written as zeros");
    }
    return dst;
}

}  // namespace

// ---- the trainer's per-iteration bookkeeping (gsr_masked_max / gsr_densify_stats_add / gsr_psnr; include/gsr.h) ------------------
void masked_max_(Tensor dst, const Tensor& src, const Tensor& mask)
{
    TORCH_CHECK(dst.is_cuda(), "masked_max_: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dst.device());
    TORCH_CHECK(dst.is_contiguous() && dst.scalar_type() == at::kFloat && src.is_contiguous() && src.scalar_type() == at::kInt &&
                mask.is_contiguous() && mask.scalar_type() == at::kBool && dst.dim() == 1 && src.numel() == dst.numel() && mask.numel() == dst.numel(),
                "masked_max_: dst float32 [n], src int32 [n], mask bool [n], contiguous");
    check(gsr_masked_max(dst.data_ptr<float>(), src.data_ptr<int32_t>(), reinterpret_cast<const uint8_t*>(mask.data_ptr<bool>()), (int32_t)dst.numel(),
                         c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_masked_max");
    torch::autograd::impl::bump_version(dst);
}

void densify_stats_add_(Tensor accum, Tensor denom, const Tensor& grad, const Tensor& mask)
{
    TORCH_CHECK(accum.is_cuda(), "densify_stats_add_: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(accum.device());
    const int64_t n = mask.numel();
    TORCH_CHECK(accum.is_contiguous() && denom.is_contiguous() && grad.is_contiguous() && mask.is_contiguous() && accum.scalar_type() == at::kFloat &&
                denom.scalar_type() == at::kFloat && grad.scalar_type() == at::kFloat && mask.scalar_type() == at::kBool && accum.numel() == n &&
                denom.numel() == n && grad.numel() == 3 * n, "densify_stats_add_: accum / denom float32 [n(,1)], grad float32 [n,3], mask bool [n], contiguous");
    check(gsr_densify_stats_add(accum.data_ptr<float>(), denom.data_ptr<float>(), grad.data_ptr<float>(),
                                reinterpret_cast<const uint8_t*>(mask.data_ptr<bool>()), (int32_t)n,
                                c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_densify_stats_add");
    torch::autograd::impl::bump_version(accum);
    torch::autograd::impl::bump_version(denom);
}

// gsr::batch_retire -> gsr_batch_retire: the per-model exit decision on the render a step just produced.  render / target: [B,C,H,W] (or
// [C,H,W] for one model); retired_at: B int32 entries, updated in place on the stream; returns the images' MSEs (B doubles, device).  No host
// synchronisation.
Tensor batch_retire(const Tensor& render_, const Tensor& target_, Tensor retired_at, double mse_bar, int64_t exit_after, int64_t step)
{
    TORCH_CHECK(render_.is_cuda() && target_.is_cuda() && retired_at.is_cuda(), "batch_retire: tensors must be on a ROCm/HIP device (no CPU fallback)");
    TORCH_CHECK((render_.dim() == 3 || render_.dim() == 4) && render_.numel() == target_.numel(), "batch_retire: render and target are [B,C,H,W] stacks (or [C,H,W]) of one size");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(render_.device());
    const Tensor render = f32c(render_.detach()), target = f32c(target_.detach());
    const int64_t B = render.dim() == 4 ? render.size(0) : 1, C = render.size(-3), H = render.size(-2), W = render.size(-1);
    TORCH_CHECK(retired_at.scalar_type() == at::kInt && retired_at.is_contiguous() && retired_at.numel() == B,
                "batch_retire: retired_at must be a contiguous int32 tensor with one entry per image");
    Tensor mse = at::empty({B}, render.options().dtype(at::kDouble));
    Tensor scratch = at::empty({(int64_t)gsr_batch_retire_scratch_bytes((int32_t)B)}, render.options().dtype(at::kByte));
    const int rc = gsr_batch_retire(render.data_ptr<float>(), target.data_ptr<float>(), (int32_t)B, (int32_t)C, (int32_t)H, (int32_t)W, mse_bar, exit_after, step,
                                    retired_at.data_ptr<int32_t>(), mse.data_ptr<double>(), scratch.data_ptr(),
                                    c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream());
    TORCH_CHECK(rc == 0, "gsr_batch_retire failed (code ", rc, "): step >= 1, exit_after >= 0 and at most 65535 images expected");
    return mse;
}

Tensor psnr(const Tensor& a, const Tensor& b)
{
    TORCH_CHECK(a.is_cuda(), "psnr: tensors must be on a ROCm/HIP device (no CPU fallback)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(a.device());
    const Tensor x = f32c(a), y = f32c(b);
    TORCH_CHECK(x.dim() >= 2 && x.sizes() == y.sizes(), "psnr: two images of the same shape [C, ...]");
    const int64_t C = x.size(0), P = x.numel() / C;
    Tensor out = at::empty({C, 1}, x.options());
    Tensor scratch = at::empty({(int64_t)gsr_psnr_scratch_bytes((int32_t)C)}, x.options().dtype(at::kByte));
    check(gsr_psnr(x.data_ptr<float>(), y.data_ptr<float>(), (int32_t)C, P, out.data_ptr<float>(), scratch.data_ptr(),
                   c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()), "gsr_psnr");
    return out;
}

TORCH_LIBRARY(gsr, m)
{
    m.def("rasterize_forward(Tensor means3D, Tensor sh, Tensor colors_precomp, Tensor opacities, Tensor scales, Tensor rotations, "
          "Tensor cov3D_precomp, Tensor sh_rest, Tensor viewmatrix, Tensor projmatrix, Tensor campos, Tensor bg, Tensor points_transform, "
          "int image_height, int image_width, float tanfovx, float tanfovy, float scale_modifier, int sh_degree, bool raw_params, "
          "bool prefiltered, bool debug, Tensor prepared, int[] batch_first_block, int view_id=0, int extras=0, Tensor? sh_origin=None) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("rasterize_backward(Tensor means3D, Tensor sh, Tensor colors_precomp, Tensor opacities, Tensor scales, Tensor rotations, "
          "Tensor cov3D_precomp, Tensor sh_rest, Tensor viewmatrix, Tensor projmatrix, Tensor campos, Tensor bg, Tensor points_transform, "
          "Tensor geom, Tensor image, Tensor binning, Tensor meta, Tensor grad_color, Tensor grad_depth, Tensor grad_alpha, "
          "int image_height, int image_width, float tanfovx, float tanfovy, float scale_modifier, int sh_degree, bool raw_params, "
          "bool need_viewmatrix, bool need_projmatrix, bool need_campos, bool need_points_transform, Tensor(a!)[] densify_stats, Tensor radii, int[] batch_first_block, "
          "Tensor? sh_origin=None) -> Tensor[]");
    m.def("rasterize_backward_frozen(Tensor means3D, Tensor sh, Tensor colors_precomp, Tensor opacities, Tensor scales, Tensor rotations, "
          "Tensor cov3D_precomp, Tensor sh_rest, Tensor viewmatrix, Tensor projmatrix, Tensor campos, Tensor bg, Tensor points_transform, "
          "Tensor geom, Tensor image, Tensor binning, Tensor meta, Tensor grad_color, Tensor grad_depth, Tensor grad_alpha, "
          "int image_height, int image_width, float tanfovx, float tanfovy, float scale_modifier, int sh_degree, bool raw_params, "
          "bool need_means2D, bool need_viewmatrix, bool need_projmatrix, bool need_campos, bool need_points_transform, int[] batch_first_block, "
          "Tensor? sh_origin=None) -> Tensor[]");
    m.def("rasterize_backward_views(Tensor means3D, Tensor sh, Tensor colors_precomp, Tensor opacities, Tensor scales, Tensor rotations, "
          "Tensor cov3D_precomp, Tensor sh_rest, Tensor viewmatrix, Tensor projmatrix, Tensor campos, Tensor bg, Tensor points_transform, "
          "Tensor geom, Tensor image, Tensor binning, Tensor meta, Tensor grad_color, Tensor grad_depth, Tensor grad_alpha, "
          "int image_height, int image_width, float tanfovx, float tanfovy, float scale_modifier, int sh_degree, bool raw_params, "
          "bool need_means2D, bool need_viewmatrix, bool need_projmatrix, bool need_campos, bool need_points_transform, "
          "Tensor? sh_origin=None) -> Tensor[]");
    m.def("rasterize_backward_fused(Tensor(a!) means3D, Tensor(b!) sh, Tensor(c!) sh_rest, Tensor(d!) opacities, Tensor(e!) scales, "
          "Tensor(f!) rotations, Tensor viewmatrix, Tensor projmatrix, Tensor campos, Tensor bg, Tensor points_transform, Tensor geom, "
          "Tensor image, Tensor binning, Tensor meta, Tensor grad_color, Tensor grad_depth, Tensor grad_alpha, int image_height, "
          "int image_width, float tanfovx, float tanfovy, float scale_modifier, int sh_degree, bool need_viewmatrix, bool need_projmatrix, "
          "bool need_campos, bool need_points_transform, Tensor(g!)[] adam_m, Tensor(h!)[] adam_v, float[] adam_lr, float beta1, "
          "float beta2, float eps, int step, Tensor next_viewmatrix, Tensor next_projmatrix, Tensor next_campos, int next_height, "
          "int next_width, float next_tanfovx, float next_tanfovy, Tensor(i!) prepared_out, Tensor next_points_transform, int next_sh_degree, Tensor(j!)[] densify_stats, Tensor radii, int[] batch_first_block, "
          "Tensor? sh_origin=None) -> Tensor[]");
    m.def("rasterize(Tensor means3D, Tensor means2D, Tensor sh, Tensor colors_precomp, Tensor opacities, Tensor scales, Tensor rotations, "
          "Tensor cov3D_precomp, Tensor sh_rest, Tensor viewmatrix, Tensor projmatrix, Tensor campos, Tensor bg, Tensor points_transform, "
          "int image_height, int image_width, float tanfovx, float tanfovy, float scale_modifier, int sh_degree, bool raw_params, "
          "bool prefiltered, bool debug, bool cam_grad, Tensor[] adam_m, Tensor[] adam_v, float[] adam_lr, float beta1, float beta2, "
          "float eps, int step, Tensor prepared, Tensor next_viewmatrix, Tensor next_projmatrix, Tensor next_campos, int next_height, "
          "int next_width, float next_tanfovx, float next_tanfovy, Tensor next_points_transform, int next_sh_degree, Tensor adam_commit, Tensor[] densify_stats, int[] batch_first_block, int view_id=0, int extras=0, "
          "Tensor? sh_origin=None, int frozen=-1) -> "
          "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("render(Tensor means3D, Tensor sh, Tensor colors_precomp, Tensor opacities, Tensor scales, Tensor rotations, Tensor cov3D_precomp, "
          "Tensor sh_rest, Tensor viewmatrix, Tensor projmatrix, Tensor campos, Tensor bg, Tensor points_transform, int image_height, "
          "int image_width, float tanfovx, float tanfovy, float scale_modifier, int sh_degree, bool raw_params, int view_id=0, int outputs=0, "
          "Tensor? sh_origin=None) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("importance_accumulate(Tensor(a!) acc, Tensor means3D, Tensor sh, Tensor colors_precomp, Tensor opacities, Tensor scales, "
          "Tensor rotations, Tensor cov3D_precomp, Tensor sh_rest, Tensor viewmatrix, Tensor projmatrix, Tensor campos, Tensor bg, "
          "Tensor points_transform, int image_height, int image_width, float tanfovx, float tanfovy, float scale_modifier, int sh_degree, "
          "bool raw_params, int[] batch_first_block, int view_id=0, Tensor? sh_origin=None) -> Tensor[]");
    m.def("importance_pass(Tensor(a!) acc, Tensor means3D, Tensor sh, Tensor sh_rest, Tensor campos, Tensor points_transform, Tensor color, "
          "Tensor geom, Tensor image, Tensor binning, Tensor meta, int image_height, int image_width, int sh_degree, Tensor? sh_origin=None) -> ()");
    m.def("rasterize_forward_views(Tensor means3D, Tensor sh, Tensor colors_precomp, Tensor opacities, Tensor scales, Tensor rotations, "
          "Tensor cov3D_precomp, Tensor sh_rest, Tensor viewmatrix, Tensor projmatrix, Tensor campos, Tensor bg, Tensor points_transform, "
          "int image_height, int image_width, float tanfovx, float tanfovy, float scale_modifier, int sh_degree, bool raw_params, "
          "int extras=0, Tensor? sh_origin=None) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("importance_accumulate_views(Tensor(a!) acc, Tensor means3D, Tensor sh, Tensor colors_precomp, Tensor opacities, Tensor scales, "
          "Tensor rotations, Tensor cov3D_precomp, Tensor sh_rest, Tensor viewmatrix, Tensor projmatrix, Tensor campos, Tensor bg, "
          "Tensor points_transform, int image_height, int image_width, float tanfovx, float tanfovy, float scale_modifier, int sh_degree, "
          "bool raw_params, Tensor? sh_origin=None) -> Tensor[]");
    m.def("mark_visible(Tensor means3D, Tensor viewmatrix, Tensor projmatrix) -> Tensor");
    m.def("photometric_loss_forward(Tensor render, Tensor target, float lambda_dssim, bool clamp) -> (Tensor, Tensor)");
    m.def("photometric_loss_backward(Tensor render, Tensor target, Tensor workspace, Tensor grad_loss, float lambda_dssim, bool clamp) -> Tensor");
    m.def("photometric_loss(Tensor render, Tensor target, float lambda_dssim, bool clamp) -> Tensor");
    m.def("photometric_loss_terms(Tensor render, Tensor target, float lambda_dssim, bool clamp) -> (Tensor, Tensor)");
    m.def("depth_loss_forward(Tensor depth, Tensor depth_gt, int kind, float clamp_lo, float clamp_hi) -> (Tensor, Tensor)");
    m.def("depth_loss_forward_stack(Tensor depth, Tensor depth_gt, int kind, float clamp_lo, float clamp_hi) -> (Tensor, Tensor, Tensor)");
    m.def("depth_loss_backward(Tensor depth, Tensor depth_gt, Tensor workspace, Tensor grad_loss, int kind, float clamp_lo, float clamp_hi, "
          "float lambda_depth) -> Tensor");
    m.def("depth_loss(Tensor depth, Tensor depth_gt, int kind, float clamp_lo, float clamp_hi) -> Tensor");
    m.def("training_loss_terms(Tensor render, Tensor target, Tensor depth, Tensor depth_gt, float lambda_dssim, float lambda_depth, int kind, "
          "bool clamp, float clamp_lo, float clamp_hi) -> (Tensor, Tensor)");
    m.def("adam_step(Tensor(a!)[] params, Tensor[] grads, Tensor(b!)[] exp_avg, Tensor(c!)[] exp_avg_sq, float[] lr, float beta1, "
          "float beta2, float eps, int step) -> ()");
    m.def("pose_step(Tensor(a!) delta, Tensor(b!) exp_avg, Tensor(c!) exp_avg_sq, Tensor d_xf, Tensor base, Tensor(d!) xf, float lr, "
          "float beta1, float beta2, float eps, int step) -> ()");
    m.def("pose_step_many(Tensor(a!) delta, Tensor(b!) exp_avg, Tensor(c!) exp_avg_sq, Tensor d_xf, Tensor base, Tensor(d!) xf, float lr, "
          "float beta1, float beta2, float eps, int step) -> ()");
    m.def("pose_step_camera(Tensor(a!) delta, Tensor(b!) exp_avg, Tensor(c!) exp_avg_sq, Tensor d_viewmatrix, Tensor d_projmatrix, "
          "Tensor d_campos, Tensor projection_T, Tensor base, Tensor(d!) viewmatrix, Tensor(e!) projmatrix, Tensor(f!) campos, float lr, "
          "float beta1, float beta2, float eps, int step) -> ()");
    m.def("pose_matrix_forward(Tensor delta, Tensor base) -> Tensor");
    m.def("pose_matrix_backward(Tensor delta, Tensor base, Tensor d_xf) -> Tensor");
    m.def("pose_matrix(Tensor delta, Tensor base) -> Tensor");
    m.def("knn_mean_dist2(Tensor points) -> Tensor");
    m.def("depth_to_points(Tensor depth, Tensor? image, float fx, float fy, float cx, float cy) -> (Tensor, Tensor)");
    m.def("voxel_down_sample(Tensor points, Tensor? colors, float voxel_size) -> (Tensor points, Tensor colors, Tensor counts, int dropped)");
    m.def("camera_from_pose(Tensor pose, float fx, float fy, float cx, float cy, int W, int H, float znear=0.01, float zfar=100.0) -> "
          "(Tensor viewmatrix, Tensor projmatrix, Tensor campos)");
    m.def("pose_virtual_view(Tensor pose0, Tensor pose1, float alpha, Tensor? base=None) -> (Tensor out, Tensor out_rel)");
    m.def("resize_plan(Tensor flags) -> (Tensor plan, Tensor meta)");
    m.def("resize_apply(Tensor plan, Tensor(a!) meta, int N, int nA, int nB, int nC, int nSplit, Tensor[] src, int[] kinds, Tensor[] child, "
          "bool check=False) -> Tensor[]");
    m.def("resize_plan_batched(Tensor flags, int[] first_block, int[] counts) -> (Tensor plan, Tensor meta)");
    m.def("resize_apply_batched(Tensor plan, Tensor(a!) meta, int[] first_block, int[] counts, int[] counts4, int[] new_first_block, Tensor[] src, "
          "int[] kinds, Tensor[] child, Tensor[] pad, bool check=False) -> Tensor[]");
    m.def("select_smallest(Tensor values, int k) -> (Tensor drop, Tensor keep_flags, Tensor meta)");
    m.def("merge_apply(Tensor plan_a, Tensor plan_b, Tensor(a!) meta, int Na, int nA, int Nb, int nB, Tensor[] src_a, Tensor[] src_b, int[] kinds, "
          "bool check=False) -> Tensor[]");
    m.def("masked_max_(Tensor(a!) dst, Tensor src, Tensor mask) -> ()");
    m.def("densify_stats_add_(Tensor(a!) accum, Tensor(b!) denom, Tensor grad, Tensor mask) -> ()");
    m.def("psnr(Tensor a, Tensor b) -> Tensor");
    m.def("debug_last() -> Tensor[]", &debug_last);
    m.def("batch_retire(Tensor render, Tensor target, Tensor(a!) retired_at, float mse_bar, int exit_after, int step) -> Tensor");
    m.def("retire_attach(Tensor retired_at, int step) -> ()", &retire_attach);
}

TORCH_LIBRARY_IMPL(gsr, CUDA, m)   // the dispatch key of HIP tensors on a ROCm build
{
    m.impl("rasterize_forward", &rasterize_forward);
    m.impl("rasterize_backward", &rasterize_backward);
    m.impl("rasterize_backward_fused", &rasterize_backward_fused);
    m.impl("rasterize_backward_frozen", &rasterize_backward_frozen);
    m.impl("rasterize_backward_views", &rasterize_backward_views);
    m.impl("render", &render);
    m.impl("importance_accumulate", &importance_accumulate);
    m.impl("importance_pass", &importance_pass);
    m.impl("rasterize_forward_views", &rasterize_forward_views);
    m.impl("importance_accumulate_views", &importance_accumulate_views);
    m.impl("mark_visible", &mark_visible);
    m.impl("photometric_loss_forward", &photometric_loss_forward);
    m.impl("photometric_loss_backward", &photometric_loss_backward);
    m.impl("adam_step", &adam_step);
    m.impl("pose_step", &pose_step);
    m.impl("pose_step_many", &pose_step_many);
    m.impl("pose_step_camera", &pose_step_camera);
    m.impl("pose_matrix_forward", &pose_matrix_forward);
    m.impl("pose_matrix_backward", &pose_matrix_backward);
    m.impl("pose_matrix", &pose_matrix_forward);
    m.impl("knn_mean_dist2", &knn_mean_dist2);
    m.impl("depth_to_points", &depth_to_points);
    m.impl("voxel_down_sample", &voxel_down_sample);
    m.impl("camera_from_pose", &camera_from_pose);
    m.impl("pose_virtual_view", &pose_virtual_view);
    m.impl("resize_plan", &resize_plan);
    m.impl("resize_apply", &resize_apply);
    m.impl("resize_plan_batched", &resize_plan_batched);
    m.impl("resize_apply_batched", &resize_apply_batched);
    m.impl("select_smallest", &select_smallest);
    m.impl("merge_apply", &merge_apply);
    m.impl("masked_max_", &masked_max_);
    m.impl("densify_stats_add_", &densify_stats_add_);
    m.impl("psnr", &psnr);
    m.impl("batch_retire", &batch_retire);
    m.impl("rasterize", &rasterize_forward_only);
    m.impl("photometric_loss", &photometric_loss_no_grad);
    m.impl("photometric_loss_terms", &photometric_loss_terms_no_grad);
    m.impl("depth_loss_forward", &depth_loss_forward);
    m.impl("depth_loss_forward_stack", &depth_loss_forward_stack);
    m.impl("depth_loss_backward", &depth_loss_backward);
    m.impl("depth_loss", &depth_loss_no_grad);
    m.impl("training_loss_terms", &training_loss_terms_no_grad);
}

TORCH_LIBRARY_IMPL(gsr, Autograd, m)
{
    m.impl("rasterize", &rasterize);
    m.impl("photometric_loss", &photometric_loss);
    m.impl("photometric_loss_terms", &photometric_loss_terms);
    m.impl("depth_loss", &depth_loss);
    m.impl("training_loss_terms", &training_loss_terms);
    m.impl("pose_matrix", &pose_matrix);
}
