/*
 * gsr.h -- C ABI of the MI355X-native differentiable surface-Gaussian rasterizer.
 *
 * This is the drop-in boundary below the reference's Python API
 * (DGR = gaussian_splatting/submodules/diff-gaussian-rasterization).  Each entry
 * point names the reference interface it replaces.  Plain pointers, sizes and a HIP
 * stream only: no torch types, no C++ types.  All pointers are DEVICE pointers unless
 * marked [host].  All arrays are fp32 row-major and contiguous; matrices are the
 * reference's transposed (column-major) 4x4s (DGR/cuda_rasterizer/auxiliary.h:58-77).
 * "Absent" optional inputs are NULL (the reference passes data_ptr() of a 0-element
 * tensor, DGR/rasterize_points.cu:94-111).
 *
 * Ownership (as DGR/rasterize_points.cu:68-78): the caller owns every buffer including
 * the three scratch buffers, and backward re-derives its view of the scratch from
 * (P, R, W, H) alone (DGR/cuda_rasterizer/rasterizer_impl.cu:371-373).  The library itself
 * holds: per calling thread, a 64-byte pinned landing pad for the stage-1 totals and the
 * last error message; process-wide, a pool of HIP events for gsr_profile_*; and -- only
 * once gsr_forward_fused has been used -- one block of tile counters (<= 1 MB) per
 * (device, stream), exclusive to one call at a time (a concurrent call on the same
 * stream falls back to counters in its own image buffer) and freed by
 * gsr_release_stream_state().  Nothing else persists between calls.
 *
 * Every function returns 0 on success, non-zero on failure; gsr_last_error() then
 * holds a message for the calling thread.
 */
#ifndef GSR_H_INCLUDED
#define GSR_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gsr_stream_t; /* a hipStream_t; NULL = the default stream */

/* Growable-buffer callback: must return a device pointer to at least `bytes` bytes that
 * stays valid until the matching backward has run.  Mirrors the three
 * std::function<char*(size_t)> of CudaRasterizer::Rasterizer::forward
 * (DGR/cuda_rasterizer/rasterizer.h:32-34; DGR/rasterize_points.cu:27-33). */
typedef void* (*gsr_alloc_fn)(void* ctx, size_t bytes);

/* ABI version of this header (bumped on any signature change). */
int gsr_abi_version(void);

/* Message of the last failure on this thread ("" if none). */
const char* gsr_last_error(void);

/* Scratch sizes in bytes.  Replace CudaRasterizer::required<GeometryState|ImageState|
 * BinningState>() (DGR/cuda_rasterizer/rasterizer_impl.h:66-72). */
size_t gsr_geom_bytes(int P);
size_t gsr_image_bytes(int W, int H);
size_t gsr_binning_bytes(int R, int num_segments);
/* Same for a render with num_channels colour channels (3, 4 or 6, see gsr_forward_stage2_mt). */
size_t gsr_binning_bytes_mt(int R, int num_segments, int num_channels);
/* Backward-only scratch: one packed 48-byte accumulation record per Gaussian.  Takes the place of the
 * dL_dconic [P,2,2] work tensor the reference binding allocates (DGR/rasterize_points.cu:154). */
size_t gsr_grad_scratch_bytes(int P);

/* Forward, first half: per-Gaussian projection/culling/covariance/SH->RGB, tile counting and
 * the tile-offset scan; reads back num_rendered (= Gaussian x tile instances this library will
 * blend) -- the one host synchronisation of the forward, like
 * DGR/cuda_rasterizer/rasterizer_impl.cu:281.  Replaces rasterizer_impl.cu:198-281
 * (FORWARD::preprocess, forward.cu:155-256, + InclusiveSum).
 *   radii [P] int32 out (same values as the reference's), geom/image scratch sized by
 *   gsr_geom_bytes / gsr_image_bytes.  *num_rendered [host] out; *max_tile_instances [host] out =
 *   the longest per-tile list (lets stage 2 pick its LDS sort capacity without a second sync);
 *   *num_segments [host] out = number of (tile, list segment) work units of the backward pass, which
 *   also sizes the per-segment snapshot area of the binning buffer. */
int gsr_forward_stage1(int P, int D, int M, const float* means3D, const float* shs, const float* colors_precomp,
                       const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                       const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                       const float* campos, int W, int H, float tan_fovx, float tan_fovy, int prefiltered,
                       int* radii, void* geom_buffer, void* image_buffer, int* num_rendered,
                       int* max_tile_instances, int* num_segments, gsr_stream_t stream);

/* Forward, second half: instance scatter into per-tile buckets, per-tile depth sort, alpha
 * blend.  Replaces rasterizer_impl.cu:283-335 (duplicateWithKeys, SortPairs,
 * identifyTileRanges, FORWARD::render = forward.cu:261-374).
 *   out_color [3,H,W] planar; binning scratch sized by gsr_binning_bytes(R, num_segments).
 *   FORWARD-ONLY renders (no gsr_backward will follow): pass -num_segments here (binning scratch still sized with
 *   +num_segments): the per-segment snapshots the backward resumes from are not written.  With R > 0 the stage-1
 *   value of num_segments (or its negation) is REQUIRED -- it fixes the layout of the binning buffer -- and 0 is an
 *   error (ABI 9; earlier versions accepted 0 as "forward-only"). */
int gsr_forward_stage2(int P, int R, int max_tile_instances, int num_segments, int W, int H, const float* background,
                       const float* colors_precomp, void* geom_buffer, void* binning_buffer, void* image_buffer,
                       float* out_color, gsr_stream_t stream);

/* Multi-target extension (no reference counterpart: the reference fixes
 * NUM_CHANNELS = 3 at compile time, DGR/cuda_rasterizer/config.h:15, and GauSTAR renders RGB and
 * depth-as-colour in two full passes over identical geometry, gaustar_trainers/refine.py:552 and :607).
 * num_channels = 6 blends two 3-channel targets in ONE walk after ONE stage 1: colors_precomp is [P,6]
 * (required: no in-kernel SH for the extra channels), background [6], out_color [6,H,W] planar.  Channels 0-2
 * and 3-5 equal two separate 3-channel renders bit for bit.  num_channels = 4 is RGB + ONE scalar target (colors_precomp
 * [P,4], background [4], out_color [4,H,W]): GauSTAR's depth render carries the same value in its three channels and the
 * trainer reads only the first (refine.py:616), so channel 3 of a 4-channel render is that image at about the cost of a
 * 3-channel render.  num_channels = 3 is gsr_forward_stage2. */
int gsr_forward_stage2_mt(int P, int R, int max_tile_instances, int num_segments, int num_channels, int W, int H,
                          const float* background, const float* colors_precomp, void* geom_buffer, void* binning_buffer,
                          void* image_buffer, float* out_color, gsr_stream_t stream);

/* Both halves in one call over a binning buffer the caller sized IN ADVANCE from a guess (e.g. 1.25x what the last
 * view needed): when gsr_binning_bytes_mt(R, num_segments, num_channels) <= binning_capacity the library goes straight
 * from the stage-1 read-back into the stage-2 launches and sets *blended = 1 -- the GPU does not idle while the caller
 * allocates and re-enters (10-15 us per view through a Python binding).  Otherwise *blended = 0, nothing of stage 2 has
 * run, and the caller allocates exactly and calls gsr_forward_stage2[_mt] as usual.  need_backward = 0 renders
 * forward-only (see gsr_forward_stage2).  grad_scratch (may be NULL): gsr_grad_scratch_bytes(P) bytes that the
 * following gsr_backward_mt will use as its grad_scratch; when *blended = 1 (and need_backward) the forward blend has
 * cleared them on the side, and that backward may be called with grad_scratch_zeroed = 1 (once: the backward leaves
 * the contents undefined).  Same replaced reference code as the two stages
 * (DGR/cuda_rasterizer/rasterizer_impl.cu:198-335). */
int gsr_forward_fused(int P, int D, int M, int num_channels, int need_backward, const float* means3D, const float* shs,
                      const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                      const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                      const float* projmatrix, const float* campos, int W, int H, float tan_fovx, float tan_fovy,
                      int prefiltered, const float* background, int* radii, void* geom_buffer, void* image_buffer,
                      void* binning_buffer, size_t binning_capacity, void* grad_scratch, float* out_color,
                      int* num_rendered, int* max_tile_instances, int* num_segments, int* blended, gsr_stream_t stream);

/* PLANNED forward (ABI 13): gsr_forward_fused for a camera that is rendered again and again (a training rig: every camera
 * once per epoch, gaustar_trainers/refine.py:534-548).  The caller keeps, per camera, a device buffer of gsr_plan_bytes(W, H)
 * bytes (ABI 16: room for TWO plans -- the one in use and the one being built for the next view) and a plan_info block from gsr_plan_info_new() = a gsr_plan_info (below; all zero at first).  A call with state == 0
 * renders the exact way (as gsr_forward_fused) and leaves a PLAN behind (built by one extra workgroup of that view's forward
 * blend; nobody waits for it: the next call with this plan_info adopts it): per tile the place and capacity of its bucket of
 * instances (this view's count + (1/8 of it, at least 16, + 1/8 of what the largest of the tile's eight neighbours holds more -- the
 * tiles that outgrow a bucket are the few on the surface's silhouette, whose counts jump when it moves a few pixels their way) times
 * 2^level, rounded up to whole 64-entry units), the tile's first unit and a launch order; plan_info is updated.  A call with state == 1 bins BY THE PLAN: preprocess claims bucket slots and writes the
 * sort keys itself, the forward blend is queued right behind it, and the host only waits for preprocess's verdict -- no
 * tile-offset scan, no scatter pass and no host round trip between the stages; (ABI 16) such a view also RE-PLANS: the same extra
 * workgroup rides in its forward blend and builds the next view's plan from this view's own tile counts into the other half of the
 * plan buffer, so a camera's plan is never older than one visit however the Gaussians move between its visits (what replaces
 * DGR/cuda_rasterizer/rasterizer_impl.cu:277-317 -- InclusiveSum, the num_rendered read-back, duplicateWithKeys,
 * identifyTileRanges -- for such a view).  *planned = 1 then, and the sizes the backward needs are the plan's CAPACITIES:
 * *num_rendered = R_cap, *num_segments = U_cap (binning_capacity must hold gsr_binning_bytes_mt(R_cap, U_cap, num_channels),
 * otherwise the call takes the exact path); images are those of the exact path bit for bit, gradients to the order of the float atomics --
 * with one exception: a planned view is never SPLIT (gsr_blend_fwd.hip: lists above 1 024 entries blended in parts), whereas the exact
 * path decides that from the current view's longest list and R; a plan is only valid while its source view would not have split at
 * three quarters of its R, so the two differ only for a view whose R has fallen below that since, and then by the parts' rounding (a tile's list is
 * the same sorted list; only where it lies differs).  A view that does not fit its plan (a bucket overflows: the Gaussians
 * have moved since the plan was made) is detected by preprocess before anything is blended; the same call then renders it the
 * exact way and re-plans with the slack level raised by one, at most 3 (*planned = -1; 0: no plan was tried).  Only views whose longest list stays within the forward blend's own sort (2 048
 * entries incl. slack) and that would not be split are planned (state stays 0 otherwise).  A plan is a HINT: any plan of
 * the right image size is safe for any view -- a bad one costs the fallback, never a wrong pixel.  Needs the library's
 * per-stream counter block (gsr_forward_fused's), otherwise exact.  All other arguments as gsr_forward_fused. */
#define GSR_PLAN_INFO_INTS 32
size_t gsr_plan_bytes(int W, int H);
/* A plan_info block: GSR_PLAN_INFO_INTS ints of pinned, device-mapped host memory, zeroed (the builder of a plan writes its
 * header there from the device; ordinary host memory will not do), laid out as this struct.  The caller reads and writes the
 * first five fields; the rest belongs to the library.  Free with gsr_plan_info_free once no call using it is in flight. */
typedef struct gsr_plan_info {
    int state;         /* 0 no plan, 1 valid, -1 this camera's views cannot be planned (reset to 0 to have the next view try again) */
    int R_cap;         /* of a valid plan: entries, */
    int U_cap;         /*   64-entry units (R_cap / 64) */
    int max_cap;       /*   and the largest bucket */
    int level;         /* slack level (0..3) */
    int half;          /* the half of the plan buffer in use */
    int pending_half;  /*   and the one the builder on its way writes */
    int reserved0;
    int header[8];     /* of the arriving plan, as its builder wrote it: valid, T, R_cap, U_cap, max_cap, non-empty tiles, entries,
                        * longest list of its source view */
    int arrived;       /* the builder's sequence number, written behind the header */
    int pending;       /* the sequence number the host expects there (0: no plan under way) */
    int diag[4];       /* (GSR_PLAN_DIAG builds) how a view sat in the plan it replaces: tiles over an empty bucket, over a non-empty
                        * one, entries over, worst count / capacity in 1/64 */
    int reserved1[10]; /* [0]: behind the arriving header, the number of LIGHT tiles at the end of that plan's launch order (capacity 0:
                        * empty with eight empty neighbours; the planned forward blend fills them many to a workgroup); [1]: that
                        * count of the plan in use; the rest is unused */
} gsr_plan_info;
int* gsr_plan_info_new(void);
void gsr_plan_info_free(int* plan_info);
int gsr_forward_planned(int P, int D, int M, int num_channels, int need_backward, const float* means3D, const float* shs,
                        const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                        const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                        const float* projmatrix, const float* campos, int W, int H, float tan_fovx, float tan_fovy,
                        int prefiltered, const float* background, int* radii, void* geom_buffer, void* image_buffer,
                        void* binning_buffer, size_t binning_capacity, void* grad_scratch, float* out_color,
                        int* num_rendered, int* max_tile_instances, int* num_segments, int* blended, void* plan_buffer,
                        int* plan_info, int* planned, gsr_stream_t stream);

/* CONTENT key of a camera (ABI 15): a 64-bit hash of the sixteen floats of its view matrix, read from wherever the caller
 * keeps them (row_stride / col_stride in elements: the reference hands over a TRANSPOSED view,
 * gaustar_scene/sugar_model.py:1149-1150).  What a caller keys its per-camera plans on when it cannot know the camera any other
 * way: the reference's caller builds a fresh view-matrix tensor on every render call (sugar_model.py:1149-1163), so neither the
 * tensor nor its address identifies the camera -- its contents do.  The sixteen floats are fetched by a one-wave kernel on a
 * library-owned NON-BLOCKING stream into the calling thread's pinned pad and the host waits for that kernel only: the caller's
 * stream is neither waited for nor delayed (work queued on it keeps running underneath).  The read is therefore not ordered
 * behind kernels of the caller's stream that may still be writing the matrix; a matrix uploaded from the host (the reference's
 * case: `.cuda()` synchronises) or resident since an earlier call is final.  A key of half-written contents is harmless -- a
 * plan is a hint (gsr_forward_planned) -- it merely names no camera. */
int gsr_camera_key(const float* viewmatrix, long long row_stride, long long col_stride, unsigned long long* key);
/* The same in two halves, so that the caller's own host work (allocating the view's buffers) hides the ~10 us round trip:
 * _begin launches the read, _end (same host thread, once per _begin) waits for it and returns the key. */
int gsr_camera_key_begin(const float* viewmatrix, long long row_stride, long long col_stride);
int gsr_camera_key_end(unsigned long long* key);

/* Frees what the library keeps for (current device, stream) -- the tile-counter block of gsr_forward_fused -- e.g.
 * before the stream is destroyed.  Fails if a gsr_forward_fused on that stream is in flight on another thread. */
int gsr_release_stream_state(gsr_stream_t stream);

/* One-call forward with the reference's allocator-callback shape.  Replaces
 * CudaRasterizer::Rasterizer::forward (DGR/cuda_rasterizer/rasterizer.h:31-55).
 * Returns num_rendered through *num_rendered [host]. */
int gsr_forward(gsr_alloc_fn geometry_buffer, gsr_alloc_fn binning_buffer, gsr_alloc_fn image_buffer, void* alloc_ctx,
                int P, int D, int M, const float* background, int W, int H, const float* means3D, const float* shs,
                const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                const float* campos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color, int* radii,
                int* num_rendered, gsr_stream_t stream);

/* Backward.  Replaces CudaRasterizer::Rasterizer::backward
 * (DGR/cuda_rasterizer/rasterizer.h:57-83; rasterizer_impl.cu:340-434; backward.cu).
 * Output gradient arrays need NOT be zeroed by the caller (the reference requires zeroed
 * tensors, DGR/rasterize_points.cu:151-159; here the fill is part of the call):
 *   grad_scratch: gsr_grad_scratch_bytes(P) bytes of work space (contents undefined afterwards);
 *   dL_dmean2D [P,3], dL_dopacity [P], dL_dcolor [P,3], dL_dmean3D [P,3], dL_dcov3D [P,6] (may be NULL when
 *   cov3D_precomp is NULL: the reference writes it regardless, rasterizer_impl.cu:401-416, and its binding then drops it),
 *   dL_dsh [P,M,3] (NULL when M == 0), dL_dscale [P,3], dL_drot [P,4] (both NULL when cov3D_precomp
 *   is given). */
int gsr_backward(int P, int D, int M, int R, int num_segments, const float* background, int W, int H,
                 const float* means3D, const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                 const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                 const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                 const void* geom_buffer, const void* binning_buffer, const void* image_buffer, const float* dL_dpix,
                 void* grad_scratch, float* dL_dmean2D, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                 float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, gsr_stream_t stream);

/* Backward of a num_channels render (see gsr_forward_stage2_mt): dL_dpix [num_channels,H,W], dL_dcolor
 * [P,num_channels]; every other gradient is the sum over the targets, i.e. what autograd would accumulate from
 * the separate backward passes of the reference.  num_channels = 3 is gsr_backward.
 * Precision of the per-pixel sums: f32 products and f32 sums for every channel of every channel count (ABI 16; the four-channel
 * kernel of ABI 13-15 took dL_dpix of channels 2 and 3 into the matrix pipe with 16 mantissa bits).
 * grad_scratch_zeroed = 1: the caller guarantees grad_scratch is all zero (gsr_forward_fused cleared it) and the
 * library skips its own fill; 0: the fill is part of the call, as in gsr_backward. */
int gsr_backward_mt(int P, int D, int M, int R, int num_segments, int num_channels, const float* background, int W,
                    int H, const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                    float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                    const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                    const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                    const float* dL_dpix, void* grad_scratch, float* dL_dmean2D, float* dL_dopacity, float* dL_dcolor,
                    float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                    int grad_scratch_zeroed, gsr_stream_t stream);

/* Near-plane visibility test.  Replaces CudaRasterizer::Rasterizer::markVisible
 * (DGR/cuda_rasterizer/rasterizer.h:24-29; rasterizer_impl.cu:54-66, :141-153).
 * present [P] uint8 (bool) out. */
int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, gsr_stream_t stream);

/* Introspection for tests/benchmarks: copies library-internal per-stage results out of the
 * scratch buffers into caller-provided DEVICE arrays (any may be NULL):
 *   means2D [P,2], conic_opacity [P,4], depths [P], rgb [P,3] (SH mode only),
 *   tile_ranges [T,2] uint32, point_list [R] uint32, final_T [H*W], n_contrib [H*W] uint32.
 * No reference counterpart (the reference exposes its scratch only as opaque bytes). */
int gsr_debug_export(int P, int R, int num_segments, int W, int H, const void* geom_buffer, const void* binning_buffer,
                     const void* image_buffer, float* means2D, float* conic_opacity, float* depths, float* rgb,
                     uint32_t* tile_ranges, uint32_t* point_list, float* final_T, uint32_t* n_contrib,
                     gsr_stream_t stream);
/* Same for the per-pixel candidate words of the binning buffer: masks [num_segments][4][64] uint64 -- unit (= 64-entry
 * segment of a tile's list; units of a tile are consecutive, tiles in index order), 8x8 block 2*by + bx of the tile, pixel
 * 8*(y % 8) + (x % 8) of the block.  Bit i of a word <=> the instance at list position 64*segment + i CAN reach
 * alpha >= 1/255 at that pixel (a conservative superset of what the pixel blends; bits of positions past the end of the
 * list are zero).  Words of segments the forward never reached (every pixel of the tile saturated before) are undefined.
 * No reference counterpart. */
int gsr_debug_export_masks(int R, int num_segments, const void* binning_buffer, uint64_t* masks, gsr_stream_t stream);
/* Same for the backward's unit table and the forward's live flags, which the table carries above the tile number (either may be
 * null): unit_info [num_segments][4] uint32 {tile, first list entry of the tile, entries of the tile, first unit of the tile};
 * unit_live [num_segments][4] uint8, one byte per (unit, 8x8 block): 0 <=> no pixel of the block blended an instance of the unit
 * -- the backward's wave for that pair leaves at once (GSR_BWD_LIVE=0: the flags are ignored) --, 1 <=> some pixel did, or the
 * forward does not tell (lists above 2 048 entries, tiles blended in parts).  Defined after a forward that keeps backward state,
 * for the units of the view's tiles (planned views: of their whole buckets).  No reference counterpart. */
int gsr_debug_export_units(int R, int num_segments, const void* binning_buffer, uint32_t* unit_info, uint8_t* unit_live,
                           gsr_stream_t stream);

/* ---- Producers of rasterizer inputs.
 * gsr_sh_to_rgb replaces SuGaR.get_points_rgb (gaustar_scene/sugar_model.py:674-718):
 *   rgb = clamp_min(eval_sh(D, sh[:, :(D+1)^2], normalize(positions - campos)) + 0.5, 0)
 * (eval_sh: gaustar_utils/spherical_harmonics.py:117-172); gsr_sh_to_rgb_backward is its autograd backward.
 *   positions [P,3], campos [3], shs [P,M,3] with (D+1)^2 <= M, D in 0..3; rgb / dL_drgb [P,3];
 *   dL_dsh [P,M,3] (zero above the active degree), dL_dpos [P,3] -- both written outright. */
int gsr_sh_to_rgb(int P, int D, int M, const float* positions, const float* campos, const float* shs, float* rgb,
                  gsr_stream_t stream);
int gsr_sh_to_rgb_backward(int P, int D, int M, const float* positions, const float* campos, const float* shs,
                           const float* dL_drgb, float* dL_dsh, float* dL_dpos, gsr_stream_t stream);

/* Two-target variant for the one-pass RGB + depth render (gsr_forward_stage2_mt with 6 channels): colors6 [P,6] =
 * {rgb as gsr_sh_to_rgb, z, z, z} with z = the view-space depth of the position, i.e. the `point_depth.expand(-1, 3)`
 * GauSTAR renders as colours (gaustar_trainers/refine.py:603-605: world-to-view transform of sugar.points, component 2).
 * viewmatrix [4,4] as handed to the rasterizer (row-vector convention: z = (p, 1) . column 2).  The backward adds the
 * depth channels' gradient to dL_dpos.  depth_channels = 3: [P,6] as above; 1: [P,4] = {rgb, z}, for the 4-channel render
 * (the trainer only reads channel 0 of its depth render, refine.py:616).  Replaces torch.cat + two skinny GEMMs + their
 * autograd mirror per iteration. */
int gsr_sh_to_rgbd(int P, int D, int M, const float* positions, const float* campos, const float* shs,
                   const float* viewmatrix, int depth_channels, float* colors6, gsr_stream_t stream);
int gsr_sh_to_rgbd_backward(int P, int D, int M, const float* positions, const float* campos, const float* shs,
                            const float* viewmatrix, int depth_channels, const float* dL_dcolors6, float* dL_dsh,
                            float* dL_dpos, gsr_stream_t stream);

/* The same producer reading SuGaR's coefficients where they live: `_sh_coordinates_dc` [P,1,3] and `_sh_coordinates_rest`
 * [P,M-1,3] (gaustar_scene/sugar_model.py:449-450 concatenates the two on EVERY access of `sh_coordinates`, and autograd
 * splits the gradient again: 53 MB written and read back each way per render at 491 520 Gaussians, sh_levels 3), and
 * taking SuGaR.strengths (sugar_model.py:442-447: sigmoid of `all_densities`) along.
 *   M = 1 + number of rest coefficients (sh_rest may be NULL when M == 1); viewmatrix NULL: colors [P,3], depth_channels
 *   must be 0; otherwise colors [P, 3 + depth_channels] as gsr_sh_to_rgbd.  densities / opacity [P]: both NULL or both
 *   given, opacity = 1 / (1 + exp(-density)).
 * Backward: dL_dsh_dc [P,1,3] and dL_dsh_rest [P,M-1,3] written outright; dL_dpos [P,3] written, or -- accumulate_pos != 0
 * -- ADDED to what the array holds (the rasterizer's gradient w.r.t. the same positions: the sum autograd would form with
 * one more kernel); opacity / dL_dopacity / dL_ddensities [P]: all NULL or all given, dL_ddensities = dL_dopacity (1 - o) o.
 * Results are bit-identical to gsr_sh_to_rgbd on the concatenated array + torch.sigmoid. */
int gsr_sh_colors_split(int P, int D, int M, const float* positions, const float* campos, const float* sh_dc,
                        const float* sh_rest, const float* viewmatrix, int depth_channels, const float* densities,
                        float* colors, float* opacity, gsr_stream_t stream);
int gsr_sh_colors_split_backward(int P, int D, int M, const float* positions, const float* campos, const float* sh_dc,
                                 const float* sh_rest, const float* viewmatrix, int depth_channels, const float* dL_dcolors,
                                 const float* opacity, const float* dL_dopacity, float* dL_dsh_dc, float* dL_dsh_rest,
                                 float* dL_dpos, int accumulate_pos, float* dL_ddensities, gsr_stream_t stream);

/* gsr_mesh_gaussians replaces the properties SuGaR.points / .scaling / .quaternions for Gaussians bound to a
 * triangle mesh (gaustar_scene/sugar_model.py:417-435, :457-476, :478-508; pytorch3d 0.7.4 face normals,
 * quaternion_to_matrix, matrix_to_quaternion): Gaussian n = f*G + g of face f gets
 *   points[n]  = sum_k bary[g][k] * verts[faces[f][k]]  (+ delta_t[n]),
 *   scaling[n] = {thickness, clamp(exp(raw_scales[n]), min_scale, max_scale)},
 *   quaternions[n] = normalize(matrix_to_quaternion(R(delta_r[n]) * [n_f | R1 | R2])),  (w, x, y, z),
 * with [R1 R2] the face's (first edge, normal x edge) basis turned by normalize(raw_complex[n]).
 *   verts [V,3] f32, faces [F,3] int64, bary [G,3], raw_scales / raw_complex [F*G,2]; delta_t [F*G,3] and
 *   delta_r [F*G,4] are the loose-bind offsets and may be NULL; min_scale / max_scale: -inf / +inf for "none".
 * gsr_mesh_gaussians_backward is its autograd backward: dL_dverts [V,3] is zeroed and accumulated inside;
 * dL_draw_scales, dL_draw_complex (and dL_ddelta_t, dL_ddelta_r when non-NULL) are written outright; any of
 * the three incoming gradients may be NULL (= zero).
 * (ABI 14) clear_dL_dverts / V of the forward: when non-NULL, the forward's launch also sets those [V,3] floats to zero -- the
 * accumulator of the backward to come, which is then called with dL_dverts_cleared = 1 and skips its own fill (a launch of its
 * own on the stream for 0.5 MB).  NULL / dL_dverts_cleared = 0: as before. */
int gsr_mesh_gaussians(int F, int G, const float* verts, const long long* faces, const float* bary,
                       const float* raw_scales, const float* raw_complex, float thickness, float min_scale,
                       float max_scale, const float* delta_t, const float* delta_r, float* points, float* scaling,
                       float* quaternions, float* clear_dL_dverts, int V, gsr_stream_t stream);
int gsr_mesh_gaussians_backward(int F, int G, int V, const float* verts, const long long* faces, const float* bary,
                                const float* raw_scales, const float* raw_complex, float min_scale, float max_scale,
                                const float* delta_r, const float* dL_dpoints, const float* dL_dscaling,
                                const float* dL_dquaternions, float* dL_dverts, float* dL_draw_scales,
                                float* dL_draw_complex, float* dL_ddelta_t, float* dL_ddelta_r, int dL_dverts_cleared,
                                gsr_stream_t stream);

/* ---- Image-space losses either side of the rasterizer.
 * gsr_l1_ssim replaces  (1 - f) * l1_loss(pred, gt) + f * (1 - ssim(pred, gt))  (gaustar_trainers/refine.py:451-453
 * over gaustar_utils/loss_utils.py:17-62: 11x11 Gaussian window, sigma 1.5, zero padding, mean over all
 * elements) AND its autograd backward w.r.t. pred, in two tiled passes.  Images are indexed [C,H,W] through
 * element strides (channel, row, column), so the reference's transposed views of [H,W,3] storage and its
 * margin crop (refine.py:584-594: pass pointers to the crop origin and the cropped H, W) need no copy.
 *   loss_out [3] device floats: {loss, l1 mean, ssim mean};  dL_dpred may be NULL (value only), else it receives
 *   d loss / d pred for the H x W region through its own strides (planar [C,H,W] is what gsr_backward reads).
 *   workspace: gsr_l1_ssim_workspace_bytes(C, H, W) bytes.  No host synchronisation. */
size_t gsr_l1_ssim_workspace_bytes(int C, int H, int W);
int gsr_l1_ssim(int C, int H, int W, const float* pred, long long pred_sc, long long pred_sy, long long pred_sx,
                const float* gt, long long gt_sc, long long gt_sy, long long gt_sx, float dssim_factor,
                void* workspace, float* loss_out, float* dL_dpred, long long grad_sc, long long grad_sy,
                long long grad_sx, gsr_stream_t stream);

/* Masked depth + silhouette L1 of gaustar_trainers/refine.py:634-660 (depth_alpha = False branch):
 *   depth_factor * mean_{gt < max_depth} |pred - gt|  +  mask_factor * mean_{gt > max_depth} |pred - max_depth|
 * on one [H,W] depth image (strided), with the gradient w.r.t. pred.
 *   loss_out [4] device floats: {depth term, mask term, #foreground, #background}. */
size_t gsr_depth_l1_workspace_bytes(void);
int gsr_depth_l1(int H, int W, const float* pred, long long pred_sy, long long pred_sx, const float* gt,
                 long long gt_sy, long long gt_sx, float max_depth, float depth_factor, float mask_factor,
                 void* workspace, float* loss_out, float* dL_dpred, long long grad_sy, long long grad_sx,
                 gsr_stream_t stream);

/* The same two losses with the gradient pass as a call of its own (ABI 12), for callers that learn the incoming
 * d(total)/d(loss) only in their backward pass (autograd's grad_output; refine.py:794 `loss.backward()`):
 *   gsr_l1_ssim(..., dL_dpred = NULL) / gsr_depth_l1(..., dL_dpred = NULL) / gsr_rgb_depth_loss evaluate the values and leave
 *   what the gradient needs in `workspace` resp. `loss_out`; gsr_l1_ssim_backward / gsr_depth_l1_backward then write
 *   grad_scale[0] * d loss / d pred, with grad_scale a DEVICE scalar (NULL = 1) -- no elementwise multiply over the image
 *   afterwards.  `workspace` / `stats` are the buffers of the value call, unmodified; pred / gt the same images.
 * gsr_rgb_depth_loss = the value passes of gsr_l1_ssim on an RGB image and of gsr_depth_l1 on a depth image with ONE
 * reduction kernel: loss_out [8] = {l1 + dssim loss, l1 mean, ssim mean, depth term, mask term, #fg, #bg, total of the
 * three terms}; loss_out + 3 is the `stats` argument of gsr_depth_l1_backward.  (ABI 14) The same eight floats are also left
 * in ssim_workspace at byte gsr_l1_ssim_workspace_bytes(C, H, W) - 256: gsr_rgb_depth_loss_backward's loss_out may point
 * there, so that a caller can hand loss_out itself to its user (who may modify it) and keep only the workspace. */
int gsr_l1_ssim_backward(int C, int H, int W, const float* pred, long long pred_sc, long long pred_sy, long long pred_sx,
                         const float* gt, long long gt_sc, long long gt_sy, long long gt_sx, float dssim_factor,
                         const void* workspace, const float* grad_scale, float* dL_dpred, long long grad_sc, long long grad_sy,
                         long long grad_sx, gsr_stream_t stream);
int gsr_depth_l1_backward(int H, int W, const float* pred, long long pred_sy, long long pred_sx, const float* gt,
                          long long gt_sy, long long gt_sx, float max_depth, float depth_factor, float mask_factor,
                          const float* stats, const float* grad_scale, float* dL_dpred, long long grad_sy, long long grad_sx,
                          gsr_stream_t stream);
int gsr_rgb_depth_loss(int C, int H, int W, const float* pred, long long pred_sc, long long pred_sy, long long pred_sx,
                       const float* gt, long long gt_sc, long long gt_sy, long long gt_sx, float dssim_factor,
                       void* ssim_workspace, int Hd, int Wd, const float* depth_pred, long long dpred_sy, long long dpred_sx,
                       const float* depth_gt, long long dgt_sy, long long dgt_sx, float max_depth, float depth_factor,
                       float mask_factor, void* depth_workspace, float* loss_out, gsr_stream_t stream);

/* Both gradient passes of gsr_rgb_depth_loss in ONE launch: loss_out is the [8] vector the value call wrote (its elements
 * 5 and 6 are the pixel counts the depth gradient divides by), ssim_workspace the value call's, unmodified. */
int gsr_rgb_depth_loss_backward(int C, int H, int W, const float* pred, long long pred_sc, long long pred_sy, long long pred_sx,
                                const float* gt, long long gt_sc, long long gt_sy, long long gt_sx, float dssim_factor,
                                const void* ssim_workspace, int Hd, int Wd, const float* depth_pred, long long dpred_sy,
                                long long dpred_sx, const float* depth_gt, long long dgt_sy, long long dgt_sx, float max_depth,
                                float depth_factor, float mask_factor, const float* loss_out, const float* grad_scale,
                                float* dL_dpred, long long grad_sc, long long grad_sy, long long grad_sx, float* dL_ddepth,
                                long long dgrad_sy, long long dgrad_sx, gsr_stream_t stream);

/* ---- Surface-mesh regularisers of a refinement iteration (gaustar_trainers/refine.py:676-706), fused.  Replaces
 *   nc_factor * pytorch3d.loss.mesh_normal_consistency(mesh)                                   (refine.py:685-688)
 * + edge_factor * ((|v0 - v1| over Meshes.edges_packed() - ref_edge_len)**2).mean()          (refine.py:690-696)
 * + area_factor * (Meshes.faces_areas_packed() - ref_area).abs().mean()                       (refine.py:698-702)
 * on ONE mesh: verts [V,3] f32.  The topology comes from the caller, built once per face tensor (gaustar_amd/meshes.py
 * MeshTopology), all int32 and contiguous:
 *   faces [F,3]; edges [E,2] (min, max) in pytorch3d's edges_packed() order; pairs [Q,4] = (e0, e1, a, b), one row per pair of
 *   faces sharing an edge (e0, e1), a / b their corners not on it (16-byte aligned); csr_offsets [V+1], csr_entries: the
 *   vertex-major incidence list, entry = element * 4 + role over the element index space pairs [0, Q), edges [Q, Q + E),
 *   faces [Q + E, Q + E + F) (role: e0 e1 a b / v0 v1 / corner).
 * A term whose factor is 0 or whose reference array (ref_edge_len [E], ref_area [F]) is NULL is skipped; a mesh without
 * pairs has nc = 0.  Per pair: 1 - cosine_similarity(n0, n1) (torch, eps 1e-8), n0 = (e1 - e0) x (a - e0),
 * n1 = -((e1 - e0) x (b - e0)), averaged over all pairs.  Face area 0.5 |(v1 - v0) x (v2 - v0)|.  Gradients at the
 * non-differentiable points follow torch (d|x|/dx = 0 at 0, d|v|/dv = 0 at v = 0): a zero-area face contributes no area
 * gradient.  How pytorch3d's own faces_areas_packed backward (a custom kernel) treats that case has not been checked.
 * gsr_mesh_reg_forward: one element pass + one fixed-order reduction, loss_out [4] device floats = {nc, edge, area, total},
 *   deterministic; workspace: gsr_mesh_reg_workspace_bytes(V, F, E, Q) bytes.  No host synchronisation.
 * gsr_mesh_reg_backward: ONE vertex-major launch, no float atomics (bitwise reproducible): dL_dverts [V,3] receives
 *   grad_scale[0] * d total / d verts (grad_scale a DEVICE scalar, NULL = 1) -- written, or with accumulate = 1 added to what
 *   is there with one rounding per element (= torch's X + fresh), e.g. the vertex gradient gsr_mesh_gaussians_backward left. */
size_t gsr_mesh_reg_workspace_bytes(int V, int F, int E, int Q);
int gsr_mesh_reg_forward(int V, int F, int E, int Q, const float* verts, const int* faces, const int* edges, const int* pairs,
                         const float* ref_edge_len, const float* ref_area, float nc_factor, float edge_factor, float area_factor,
                         void* workspace, float* loss_out, gsr_stream_t stream);
int gsr_mesh_reg_backward(int V, int F, int E, int Q, const float* verts, const int* faces, const int* edges, const int* pairs,
                          const int* csr_offsets, const int* csr_entries, const float* ref_edge_len, const float* ref_area,
                          float nc_factor, float edge_factor, float area_factor, const float* grad_scale, float* dL_dverts,
                          int accumulate, gsr_stream_t stream);

/* ---- Mesh Laplacian-smoothing loss and small-area regulariser of a refinement iteration, fused.  Replaces
 *   laplacian_factor * pytorch3d.loss.mesh_laplacian_smoothing(mesh, method)                    (refine.py:681-683)
 * + area_reg_factor * relu(mean_area / Meshes.faces_areas_packed() - 2).mean()                  (refine.py:713-718)
 * on ONE mesh: verts [V,3] f32, faces [F,3] int32.  The rules restate pytorch3d/loss/mesh_laplacian_smoothing.py and
 * pytorch3d/ops/laplacian_matrices.py (`laplacian`, `cot_laplacian`; 0.7) from memory of those sources; parity with pytorch3d
 * itself is not pinned.  The topology comes from the caller (gaustar_amd/meshes.py MeshTopology), int32 and contiguous:
 *   nbr_offsets [V+1], nbr: every vertex's edge neighbours, ascending (vertex_neighbours);
 *   vf_offsets [V+1], vf_entries [3F]: every vertex's incidences face * 3 + corner, ascending (vertex_face_csr).
 * Laplacian loss = (1 / V) sum_i |l_i| (Euclidean norm), N(i) the neighbours of i, method 0 / 1 / 2:
 *   0 uniform  l_i = (1 / |N(i)|) sum_{j in N(i)} v_j - v_i; a vertex without an edge has l_i = -v_i (pytorch3d's matrix has -1
 *              on the whole diagonal: such a vertex is pulled to the origin);
 *   1 cot      per face (a, b, c): A = |v_b - v_c|, B = |v_a - v_c|, C = |v_a - v_b|, s = (A + B + C) / 2,
 *              area = sqrt(max(s (s-A) (s-B) (s-C), 1e-12)), cot_a = (B^2 + C^2 - A^2) / area / 4 and cyclically; the face adds
 *              cot_a to w_bc and w_cb, cot_b to w_ca and w_ac, cot_c to w_ab and w_ba.  S_i = sum_j w_ij, n_i = 1 / S_i if
 *              S_i > 0, otherwise n_i = S_i (pytorch3d leaves a non-positive row sum as it is), l_i = n_i sum_j w_ij v_j - v_i;
 *   2 cotcurv  a_i = 0.25 / (sum of area over the faces at i) if that sum is > 0, otherwise 0; l_i = a_i (sum_j w_ij v_j - S_i v_i).
 * The weights are constants (no gradient through the degrees, the cotangents, the areas or the mean area); d|l|/dl = l / |l|,
 * 0 at l = 0.  Differences, cotangents and per-vertex sums are f64 from the f32 positions, rounded to f32 once at the end.
 * Area regulariser: area_f = 0.5 |(v_b - v_a) x (v_c - v_a)|, m = mean_f area_f (a constant), mean_f max(m / area_f - 2, 0), f32
 * with f64 sums.  A face of area exactly 0 makes the value +inf, as the torch composition does; its gradient contribution is
 * defined as 0 (torch gives NaN).
 * A term whose factor is 0 is skipped entirely: its passes do not run and its part is 0.
 * gsr_mesh_lap_forward: loss_out [3] device floats = {laplacian_factor * laplacian, area_reg_factor * area_reg, total};
 *   workspace: gsr_mesh_lap_workspace_bytes(V, F) bytes, 8-byte aligned; it keeps what the backward reads.  No host
 *   synchronisation.
 * gsr_mesh_lap_backward: ONE vertex-major launch over the forward's workspace (unmodified, same arguments): dL_dverts [V,3]
 *   receives grad_scale[0] * d total / d verts (grad_scale a DEVICE scalar, NULL = 1) -- written, or with accumulate = 1 added
 *   to what is there with one rounding per element (= torch's X + fresh), as gsr_mesh_reg_backward.
 * No float atomics, fixed summation orders (gsr_reduce.h for the totals): results are bitwise reproducible. */
size_t gsr_mesh_lap_workspace_bytes(int V, int F);
int gsr_mesh_lap_forward(int V, int F, const float* verts, const int* faces, const int* nbr_offsets, const int* nbr,
                         const int* vf_offsets, const int* vf_entries, int method, float laplacian_factor, float area_reg_factor,
                         void* workspace, float* loss_out, gsr_stream_t stream);
int gsr_mesh_lap_backward(int V, int F, const float* verts, const int* faces, const int* nbr_offsets, const int* nbr,
                          const int* vf_offsets, const int* vf_entries, int method, float laplacian_factor, float area_reg_factor,
                          void* workspace, const float* grad_scale, float* dL_dverts, int accumulate, gsr_stream_t stream);

/* ---- Regularisers on the Gaussians' own parameters (gaustar_trainers/refine.py:739-740, :743-748, :663-669), fused.  Replaces
 *   factor_t * (unbind_loss_weight * delta_t.abs()).mean()                                     (refine.py:739)
 * + factor_r * (unbind_loss_weight * delta_r[..., 1:].abs()).mean()                            (refine.py:740)
 * + torch.relu(min_opacity - strengths.view(-1, 1)).mean()                                     (refine.py:743-748)
 * + sh_factor * ((pre_sh_dc - sh_dc[:M]) ** 2).mean()                                          (refine.py:663-669)
 * All f32, contiguous device arrays: delta_t [N,3], delta_r [N,4] (w first), densities [N] raw (`all_densities`; strengths =
 * 1 / (1 + exp(-density)), the expression of gsr_sh_colors_split), sh_dc [N,3] (`_sh_coordinates_dc` viewed flat), pre_sh_dc
 * [M,3] with 0 <= M <= N: the tracked prefix of refine.py:667 (M == N is :669).  weight is read through two ELEMENT strides --
 * weight of Gaussian n, axis c at weight[n * w_row_stride + c * w_col_stride] -- so a [N] tensor or an expanded view (column
 * stride 0) and a materialised [N,3] array are read in place; NULL means 1.
 * A term is skipped when its input is NULL or its factor is 0 (opacity: densities == NULL; sh: either array NULL): it is 0 in
 * loss_out and touches no gradient buffer.  Means over 3N, 3N, N and 3M elements.
 * gsr_param_reg_forward: one element pass + one fixed-order reduction, loss_out [5] device floats = {loose_t, loose_r, opacity,
 *   sh, total}, each already multiplied by its factor; workspace: gsr_param_reg_workspace_bytes(N) bytes.
 * gsr_param_reg_backward: one elementwise launch; every output receives grad_scale[0] * d total / d input (grad_scale a DEVICE
 *   scalar, NULL = 1) -- written, or with accumulate = 1 added to what is there with one rounding per element (= torch's
 *   X + fresh).  Any output may be NULL.  Kinks as torch: d|x|/dx = 0 at 0, relu'(0) = 0; dL_ddelta_r[:, 0], the rows of
 *   dL_dsh_dc at or beyond M and the delta gradients of a Gaussian with weight 0 are exactly 0.
 * No host synchronisation, no float atomics: results are bitwise reproducible across calls and streams. */
size_t gsr_param_reg_workspace_bytes(int N);
int gsr_param_reg_forward(int N, int M, const float* delta_t, const float* delta_r, const float* weight, long long w_row_stride,
                          long long w_col_stride, float factor_t, float factor_r, const float* densities, float min_opacity,
                          const float* sh_dc, const float* pre_sh_dc, float sh_factor, void* workspace, float* loss_out,
                          gsr_stream_t stream);
int gsr_param_reg_backward(int N, int M, const float* delta_t, const float* delta_r, const float* weight, long long w_row_stride,
                           long long w_col_stride, float factor_t, float factor_r, const float* densities, float min_opacity,
                           const float* sh_dc, const float* pre_sh_dc, float sh_factor, const float* grad_scale,
                           float* dL_ddelta_t, float* dL_ddelta_r, float* dL_ddensities, float* dL_dsh_dc, int accumulate,
                           gsr_stream_t stream);

/* ---- Rig-wide topology-error detection (gaustar_trainers/refined_mesh.py:697-920 `detect_topo_err` with the depth term only,
 * as refine.py:720-734 calls it).  All device pointers; every call is asynchronous on `stream`, none synchronises the host,
 * and none uses float atomics (outputs are bitwise reproducible).
 * gsr_topo_view: one camera (refined_mesh.py:729-811), three launches.  depth_gt, render_depth, surface_depth [H,W] f32
 *   contiguous (the GT depth, the depth render and the solid-surface depth render, both with bg = max_depth); verts [V,3] f32;
 *   cam: [host] 14 doubles = the COLMAP world-to-camera rotation row-major (9), translation (3), fx, fy.  Writes row [V]:
 *   the vertex's depth loss min(|min(gt, max_depth) - render| (1 - edge_vis) 10, 2) where it is visible, -1 where not.
 *   Edge map: get_depth_edge(depth_gt, 3) of gaustar_tools/warp_mesh.py:120-130 (3x3 box filter, reflect-101 border),
 *   edge_vis = min(var / max(var) 1000, 1) (:792).  Projection (warp_mesh.py:57-74) in double without the principal
 *   point; lookup int(pix + 0.5), valid iff unclipped (:106-117).  Visible iff valid, |z - surface_depth| < 0.005 and
 *   edge_vis < 0.1 (:790-794).  A camera with no GT pixel below max_depth, or with max(var) = 0, sees nothing.
 *   workspace: gsr_topo_view_workspace_bytes(H, W) bytes, one per view in flight.
 * gsr_topo_aggregate: table [C,V] (the rows of all cameras, camera order) -> count [V] int32 (cameras that see the vertex),
 *   value [V] double = depth_scalar * the mean of the recorded losses where count >= min_observe, else 0 (:826-845);
 *   with detect_floor, vertices with y < ymin[0] + 0.02 get value 0 and count min_observe + 1 (:869-875; ymin a device
 *   scalar); valid [V] uint8 = count >= min_observe.
 * gsr_topo_propagate: mesh_vert_propagate (warp_mesh.py:133-155) as `sweeps` Jacobi sweeps over the symmetric neighbour list
 *   nbr_offsets [V+1], nbr (int32, trimesh vertex_neighbors): an invalid vertex with a valid neighbour takes the mean of its
 *   valid neighbours and becomes valid.  value_in / valid_in are not modified; value_out receives the result; value_tmp [V]
 *   double, valid_a / valid_b [V] uint8 are scratch.
 * gsr_topo_voxel_keys: open3d VoxelGrid::CreateFromPointCloud's voxel index of every vertex (build_voxel_from_pc,
 *   warp_mesh.py:185-197): origin = vmin - voxel_size / 2 (vmin [3] f32 device: the per-axis minimum), index =
 *   floor((v - origin) / voxel_size) in double, packed as keys [V] int64 = (ix << 42) | (iy << 21) | iz.  flags[0] (device
 *   int, zeroed by the caller) is set to 1 if an index falls outside [0, 2^21).
 * gsr_topo_voxel_interp: from the keys stably sorted (sorted_keys, order = the permutation) and voxel_id [V] int64 = the
 *   voxel of each sorted position (inclusive scan of the key changes, minus 1): per voxel the mean of its vertices' value
 *   (voxel_value [V] double) and the centre origin + (index + 0.5) voxel_size, then
 *   interpolate_in_voxel (warp_mesh.py:199-213): the 8 nearest centres by f32 squared distance (pytorch3d knn_points, ties
 *   to the lower voxel id), weights exp(-d^2 / voxel_size^2) + 1e-8, out [V] double = the weighted mean.  workspace:
 *   gsr_topo_voxel_workspace_bytes(V) bytes, 16-byte aligned.
 * gsr_topo_faces: faces [F,3] int32 -> face_colour [F] uint8 = (c0 + c1 + c2) / 3 truncated with c = int(min(255 value, 255))
 *   (trimesh vertex -> face colours, refined_mesh.py:913-915), face_loss [F] f32 = face_colour / 255 (:920). */
size_t gsr_topo_view_workspace_bytes(int H, int W);
int gsr_topo_view(int H, int W, int V, const float* verts, const float* depth_gt, const float* render_depth,
                  const float* surface_depth, float max_depth, const double* cam, void* workspace, float* row, gsr_stream_t stream);
int gsr_topo_aggregate(int C, int V, const float* table, const float* verts, const float* ymin, double depth_scalar,
                       int min_observe, int detect_floor, double* value, int* count, unsigned char* valid, gsr_stream_t stream);
int gsr_topo_propagate(int V, const int* nbr_offsets, const int* nbr, int sweeps, const double* value_in,
                       const unsigned char* valid_in, double* value_out, double* value_tmp, unsigned char* valid_a,
                       unsigned char* valid_b, gsr_stream_t stream);
int gsr_topo_voxel_keys(int V, const float* verts, const float* vmin, double voxel_size, long long* keys, int* flags,
                        gsr_stream_t stream);
size_t gsr_topo_voxel_workspace_bytes(int V);
int gsr_topo_voxel_interp(int V, const float* verts, const float* vmin, double voxel_size, const long long* sorted_keys,
                          const long long* order, const long long* voxel_id, const double* value, void* workspace,
                          double* voxel_value, double* out, gsr_stream_t stream);
int gsr_topo_faces(int F, const int* faces, const double* value, unsigned char* face_colour, float* face_loss,
                   gsr_stream_t stream);

/* ---- Scene-flow mesh warping to the next frame (gaustar_tools/warp_mesh.py:216-401 `warp_mesh_using_flow`, post_processing
 * 'mesh', as train_seq.py:242-245 calls it).  All device pointers unless marked [host]; every call is asynchronous on
 * `stream`, none synchronises the host, and none uses float atomics (outputs are bitwise reproducible).
 * gsr_vertex_normals: trimesh Trimesh.vertex_normals (warp_mesh.py:291-293) of verts [V,3] double, faces [F,3] int32:
 *   per face the unit normal of cross(b - a, c - b) (zero if its norm is <= 1e-12) and the corner angles, per vertex their
 *   angle-weighted sum in ascending face order, unitised (a zero sum stays zero).  vf_offsets [V+1], vf_entries [3F] int32:
 *   the vertex's incidences face * 3 + corner, vertex-major, ascending face order.  face_scratch [F,6] double.
 *   Writes normals [V,3] double.
 * gsr_warp_view: one camera (warp_mesh.py:263-340), three launches.  depth_cur, depth_next [H,W] f32 (frames f and
 *   f + interval); flow_f, flow_b: the raw RAFT flows [h,w,2] f32 in (x, y) order; flow_shape: [host] 6 ints = h, w and the
 *   zero padding top, bottom, left, right (pad.txt truncated to int32; zeros when there is none).  pad_and_resize_flow
 *   (:96-103) is fused into the reads: scale f32(H / h_padded), nearest source pixel min(floor(x / (W / w_padded)),
 *   w_padded - 1) per axis.  Edge maps: get_depth_edge(depth, 7) (:120-130, 7x7 box filter, reflect-101 border),
 *   edge_vis = min(var / max(var) edge_scalar, 1) in f32 (:298, :313).  cam: [host] 14 doubles = the COLMAP world-to-camera
 *   rotation row-major (9), translation (3), fx, fy.  params: [host] 6 doubles = warp_config's cmr_view_max_cos,
 *   edge_scalar, edge_threshold, bi_direct_depth_threshold, bi_direct_pix_threshold, max_move_dist (:14-25).  verts [V,3]
 *   double, normals [V,3] double (gsr_vertex_normals).  Writes row [V,3] double: the vertex's move where it passes every
 *   test of :295-328 (valid lookup, |z - depth_cur| < 0.005, camera-space normal z < cmr_view_max_cos, edge_vis <
 *   edge_threshold, the f32 depth and f64 pixel round trips, edge_vis of the next frame, a valid depth_next below 10 and
 *   |move| < max_move_dist), NaN in all three where it does not.  A camera with no depth below 10, or with max(var) = 0, in
 *   either frame sees nothing.  workspace: gsr_warp_view_workspace_bytes(H, W) bytes, one per view in flight.
 * gsr_warp_aggregate: table [C,V,3] (the rows of all cameras, camera order) -> observed [V] int32 (cameras that see the
 *   vertex), count [V] int32 (after remove_outlier, :174-181 and :351-358; = observed where observed < min_observe), move
 *   [V,3] double = the mean of the kept moves where count >= min_observe, else 0; valid [V] uint8 = count >= min_observe.
 *   Propagation (:384) is gsr_topo_propagate on each component with this valid mask.
 * gsr_warp_smooth: mesh_color_smoothing (:158-171) as `sweeps` Jacobi sweeps over value [V,3] double and the neighbour list
 *   of gsr_topo_propagate: every vertex takes the mean of all its neighbours; one without neighbours becomes NaN.  value_in
 *   is not modified; value_out receives the result; value_tmp [V,3] double is scratch. */
int gsr_vertex_normals(int V, int F, const double* verts, const int* faces, const int* vf_offsets, const int* vf_entries,
                       double* face_scratch, double* normals, gsr_stream_t stream);
size_t gsr_warp_view_workspace_bytes(int H, int W);
int gsr_warp_view(int H, int W, int V, const double* verts, const double* normals, const float* flow_f, const float* flow_b,
                  const int* flow_shape, const float* depth_cur, const float* depth_next, const double* cam,
                  const double* params, void* workspace, double* row, gsr_stream_t stream);
int gsr_warp_aggregate(int C, int V, const double* table, int min_observe, double* move, int* observed, int* count,
                       unsigned char* valid, gsr_stream_t stream);
int gsr_warp_smooth(int V, const int* nbr_offsets, const int* nbr, int sweeps, const double* value_in, double* value_out,
                    double* value_tmp, gsr_stream_t stream);

/* ---- A mesh's depth map, mask and visible face for one camera of the rig (data_process/render_depth_from_mesh.py:13-101
 * `render_mesh_depth_w_aitviewer`, which renders them with OpenGL): the `img_{c:04d}_depth.npz` / `_alpha.png` inputs of the
 * depth and mask losses, of detect_topo_err and of warp_mesh_using_flow.  A depth-only triangle rasterizer by the rules
 * restated in tests/meshdepth_ref.py (aitviewer was not available: parity with it is not pinned), all in double:
 *   cam16: [host] 16 doubles = gsr_warp_view's 14 (rotation row-major, translation, fx, fy) and the principal point cx, cy.
 *   local = R p + t, x = fx (lx / lz) + cx, y = fy (ly / lz) + cy; the centre of pixel (row r, column c) is at (x, y) = (c, r),
 *   the convention of gsr_topo_view / gsr_warp_view's lookups.  verts [V,3] double, faces [F,3] int32.  Skipped: a face with
 *   an index outside [0, V), with any vertex at lz <= znear (these are counted in n_clipped; nothing is clipped against the
 *   near plane) or with a zero or non-finite signed screen area.  A pixel is covered iff its three edge functions have the
 *   area's sign or are zero (inclusive edges, no culling); depth is perspective-correct, z = (float)(1 / sum_i w_i / z_i), kept
 *   iff finite and > 0; per pixel the smallest (bits(z) << 32 | face) wins: the nearest depth, ties to the lower face.
 *   Writes depth [H,W] f32 (z, or `background`), mask [H,W] uint8 (255 / 0), face_or_null [H,W] int32 (the face, or -1) and
 *   n_clipped [1] int32.  small_max: a face whose pixel range holds at most this many pixels is walked by 8 lanes, a larger
 *   one by a wave, beyond 4096 pixels by a wave per 64th of its rows (<= 0: the default, 256); the result does not depend on
 *   it.  No float atomics: the
 *   outputs are bitwise reproducible.  workspace: gsr_mesh_depth_workspace_bytes(H, W, F) bytes (8 H W + 4 F + counters), 16-byte
 *   aligned, one per view in flight.  Asynchronous on `stream`, no host read.  F == 0 yields the background image. */
size_t gsr_mesh_depth_workspace_bytes(int H, int W, int F);
int gsr_mesh_depth_view(int H, int W, int V, int F, const double* verts, const int* faces, const double* cam16, double znear,
                        float background, int small_max, void* workspace, float* depth, unsigned char* mask, int* face_or_null,
                        int* n_clipped, gsr_stream_t stream);

/* ---- A sequence's inputs before frame 0 (data_process/ahq2gaustar.py): the rectified images and the coloured base mesh.
 * All device pointers unless marked [host]; every call is asynchronous on `stream`, none synchronises the host, none uses
 * float atomics; everything is f64 in the stated order, nothing contracted (tests/prep_ref.py restates the rules in numpy).
 * gsr_image_rectify: ahq2gaustar.py:50-81 (`img_translate`, `rgb_convert`) and gaustar_tools/cmr_convert.py:71-109, :214-223
 *   (`img_convert`: cv2.undistort followed by the translation) in ONE resampling.  src, dst [H,W,C] uint8, contiguous, C in
 *   {1, 3, 4}, dst != src, H W < 2^31, any alignment.  cam4: [host] fx, fy, cx, cy; dist5_or_null: [host] k1, k2, p1, p2, k3
 *   (OpenCV's order); border: [host] C bytes.  For output pixel (row r, column c), everything in double:
 *   Plain path, taken iff dist5 is null or all five coefficients are exactly 0:
 *     su = c + (cx - 0.5 W), sv = r + (cy - 0.5 H).
 *     This is img_translate's dst(c) = src(c + dx).
 *   Distorted path:
 *     x = (c - 0.5 W) / fx, y = (r - 0.5 H) / fy, r2 = x x + y y.
 *     rad = 1 + r2 (k1 + r2 (k2 + r2 k3)).
 *     xd = x rad + (2 p1 x y + p2 (r2 + 2 x x)).
 *     yd = y rad + (p1 (r2 + 2 y y) + 2 p2 x y).
 *     su = fx xd + cx, sv = fy yd + cy.
 *   Bilinear sampling:
 *     x0 = floor(su), ax = su - x0, likewise y0, ay.
 *     The four taps are src where inside the image and border[ch] where outside (cv2's BORDER_CONSTANT).
 *     If su or sv is not finite or outside the int range, the pixel is border.
 *     Value = (t00 (1 - ax) + t01 ax) (1 - ay) + (t10 (1 - ax) + t11 ax) ay.
 *     Stored as (uint8) rint(value), half to even.
 *   Products are formed left to right; "outside the int range" is outside [-2^31, 2^31 - 1).  Departures: cv2 interpolates
 *   with 5-bit fixed-point weights and the reference resamples twice; cv2 was not available, parity with it is not pinned.
 * gsr_mesh_color_view: one camera of ahq2gaustar.py:124-160 `compute_mesh_color` (:141-151).  verts [V,3] double, image
 *   [H,W,3] uint8 RGB, depth [H,W] f32, cam14 [host] as gsr_warp_view's.  Per vertex: gsr_warp_view's projection (no principal
 *   point), row and column by its lookup int(pix + 0.5), visible = valid && fabs(lz - (double)depth[row, col]) < threshold
 *   (NaN compares false; no test on the sign of lz).  A visible vertex adds its pixel's r, g, b and 1 to sums [V,4] int32 by
 *   integer atomic adds: the sums of several cameras do not depend on their order or on the streams they ran on.
 * gsr_mesh_color_finish: :157-158 and the colours of vertices no camera saw.  sums [V,4] int32 (16-byte aligned) ->
 *   mean [V,3] double = sum / (double)n (NaN where n = 0); rgb [V,3] uint8 = (2 sum + n) / (2 n) in 64-bit integers, the mean
 *   rounded half up; filled_at [V] uint8 = 0 where n > 0.  Then fill_sweeps (0..254) Jacobi sweeps over gsr_topo_propagate's
 *   neighbour list: in sweep s = 1, 2, ... a vertex without a colour after sweep s - 1 that has k > 0 neighbours with one takes,
 *   per channel, (2 S + k) / (2 k) of those neighbours' rgb and filled_at = s; a sweep reads only the previous sweep's
 *   state.  A vertex still without a colour gets default_color ([host] 3 bytes) and filled_at = 255.  counters [2] int32:
 *   vertices with n = 0, vertices that got default_color.  The reference leaves NaN on unseen vertices; fill_sweeps = 0 keeps
 *   its seen set.  workspace: gsr_mesh_color_workspace_bytes(V) bytes, 4-byte aligned.  V == 0 is a no-op. */
int gsr_image_rectify(int H, int W, int C, const unsigned char* src, unsigned char* dst, const double* cam4,
                      const double* dist5_or_null, const unsigned char* border, gsr_stream_t stream);
int gsr_mesh_color_view(int H, int W, int V, const double* verts, const unsigned char* image, const float* depth,
                        const double* cam14, double threshold, int* sums, gsr_stream_t stream);
size_t gsr_mesh_color_workspace_bytes(int V);
int gsr_mesh_color_finish(int V, const int* sums, const int* nbr_offsets, const int* nbr, int fill_sweeps,
                          const unsigned char* default_color, void* workspace, double* mean, unsigned char* rgb,
                          unsigned char* filled_at, int* counters, gsr_stream_t stream);

/* ---- TSDF fusion of the rig's renders and mesh extraction (gaustar_trainers/refined_mesh.py:311-459 `extract_mesh_fusion`).
 * The volume follows Open3D's legacy ScalableTSDFVolume(voxel_length, sdf_trunc, RGB8) -- units of 16^3 voxels,
 * depth_sampling_stride 4 -- by the rules restated in tests/fusion_ref.py (Open3D itself was not available: parity with it
 * is not pinned), as a DENSE directory of units: grid: [host] 6 ints = the unit index floor(p / (16 voxel_size)) of the first
 * unit along x, y, z and the number of units along x, y, z.  Storage is a dense voxel grid [16 nz][16 ny][16 nx], x fastest:
 * tsdf, weight [voxels] f32 and color [3][voxels] f32 (planes R, G, B, 0..255), all zero before the first view, 16-byte
 * aligned.  What a view sees outside the grid is dropped (Open3D's hash of units is unbounded); colour is averaged in f32
 * (Open3D: double).  All device pointers unless marked [host]; every call is asynchronous on `stream`, none synchronises the
 * host, none uses float atomics: the volume is a pure function of the views and their order, the mesh of the volume.
 * cam: [host] 28 doubles = the world-to-camera matrix [R | t] (COLMAP axes, 3 rows of 4), its inverse (3 rows of 4), fx, fy,
 *   cx, cy with pixel (i, j)'s ray through ((j - cx) / fx, (i - cy) / fy, 1).
 * gsr_fusion_prep: one camera's image preparation (refined_mesh.py:412-445).  depth_alpha [3,H,W] f32: the render of the
 *   colours (z, z, 1) over a zero background; rgb [3,H,W] f32.  depth = ch0 / (alpha + 1e-8); with mask_background
 *   alpha < 0.5 -> 0; with remove_depth_edge get_depth_edge(depth, 3) of gaustar_tools/warp_mesh.py:120-130 with
 *   max_depth = None (m = 1.1 max(depth[depth < 10]), 3x3 box filter, reflect-101 border), edge_vis = min(var / max(var)
 *   1000, 1) > 0.5 -> 0 (a map with nothing below 10 or with max(var) = 0 loses nothing); depth >= depth_trunc -> 0.
 *   rgb8 [H,W,3] uint8 = clamp(rgb, 0, 1) 255 truncated.  workspace: gsr_fusion_prep_workspace_bytes(H, W) bytes.
 * gsr_fusion_touch: clears touched [units] uint8 (z, y, x order of the directory) and sets it to 1 for every unit between
 *   floor((p - sdf_trunc) / L) and floor((p + sdf_trunc) / L) per axis, L = 16 voxel_size, p = inverse(extrinsic) ((j - cx) d /
 *   fx, (i - cy) d / fy, d) for every pixel with i % 4 == 0, j % 4 == 0 and d = depth[i, j] > 0, in double.
 * gsr_fusion_integrate: over the touched units, one view into the running means.  Voxel centre = unit index L + (k + 0.5)
 *   voxel_size per axis; X = extrinsic centre in double; skipped unless X.z > 0; u_f = fx X.x / X.z + cx + 0.5 (v_f alike),
 *   skipped unless 1e-4 <= u_f < W - 1e-4 and 1e-4 <= v_f < H - 1e-4; u = (int) u_f, v = (int) v_f, d = depth[v, u], skipped
 *   unless d > 0; in f32 sdf = (d - X.z) sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1); if sdf > -sdf_trunc: t = min(1,
 *   sdf / sdf_trunc), tsdf = (tsdf w + t) / (w + 1), color = (color w + rgb8[v, u]) / (w + 1), w += 1.
 * gsr_fusion_count / gsr_fusion_emit: marching cubes over voxel centres.  A cube (its voxel = its lowest corner) is valid when
 *   all 8 weights are non-zero; corner i = (i & 1, i >> 1 & 1, i >> 2) is inside when tsdf < 0; edge e = 4 axis + j runs along
 *   `axis` from the corner whose other two coordinates (ascending axis order) are (j & 1, j >> 1) and belongs to the voxel at
 *   its lower end.  table [256,16] int32: per case up to 5 triangles as edge triples, -1 terminated (gaustar_amd.fusion.mc_table).
 *   count: edge_mask [voxels] uint8 (bit a: the edge along axis a carries a vertex -- the signs of its ends differ and one of
 *   the up to four cubes around it is valid), vert_count [voxels] int32 = its bits, tri_count [voxels] int32 = the triangles of
 *   the voxel's own cube.  emit: vert_scan / tri_scan = the INCLUSIVE scans of the counts in voxel order; a vertex sits at
 *   pa + f_a / (f_a - f_b) (pb - pa) in f32, its colour is interpolated alike and divided by 255; verts, colors [Nv,3] f32,
 *   faces [Nf,3] int32, triangles facing positive tsdf. */
size_t gsr_fusion_prep_workspace_bytes(int H, int W);
size_t gsr_fusion_volume_bytes(const int* grid);
int gsr_fusion_prep(int H, int W, const float* depth_alpha, const float* rgb, int mask_background, int remove_depth_edge,
                    float depth_trunc, void* workspace, float* depth, unsigned char* rgb8, gsr_stream_t stream);
int gsr_fusion_touch(int H, int W, const float* depth, const double* cam, double voxel_size, double sdf_trunc, const int* grid,
                     unsigned char* touched, gsr_stream_t stream);
int gsr_fusion_integrate(int H, int W, const float* depth, const unsigned char* rgb8, const double* cam, double voxel_size,
                         double sdf_trunc, const int* grid, const unsigned char* touched, float* tsdf, float* weight, float* color,
                         gsr_stream_t stream);
int gsr_fusion_count(const int* grid, const float* tsdf, const float* weight, const int* table, unsigned char* edge_mask,
                     int* vert_count, int* tri_count, gsr_stream_t stream);
int gsr_fusion_emit(const int* grid, double voxel_size, const float* tsdf, const float* color, const unsigned char* edge_mask,
                    const int* vert_scan, const int* tri_scan, const int* table, float* verts, int* faces, float* colors,
                    gsr_stream_t stream);

/* ---- Re-mesh regions at topology errors: the front half of update_mesh_topo (gaustar_trainers/refined_mesh.py:463-693) up to
 * the cuts (:516-574, :583, :609) and the primitives find_boundary_verts (:84-111) and get_outlier_cc_mask (:291-307):
 * gaustar_amd.regions.  Vertex identity is the vertex index.  faces [F,3] int32, F <= (2^31 - 1) / 3; face-edge e of face
 * (a, b, c) is (a, b), (b, c), (c, a).  All device pointers unless marked [host]; every call is asynchronous on `stream`,
 * none synchronises the host, none uses float atomics: every output is a pure function of the inputs.  err [1] int32 (zero
 * before): bit 0 is set when a face holds a vertex index outside [0, V) (a negative one, where V is not given: the calls
 * without V cannot see an index >= V); such a face is left out.  Bit 1 is set by gsr_regions_boxes when a coordinate it takes
 * into a box is NaN (the box is then not defined).
 * gsr_regions_edge_keys: selected [F] uint8 = (mask == NULL or mask[f]) and (colour == NULL or colour[f] >= cut); keys [3 F]
 *   int64 = min << 32 | max of the face-edge's vertex pair, 2^63 - 1 for the face-edges of faces that are not selected.
 * gsr_regions_edge_runs: sorted_keys = keys in ascending order, order [3 F] int64 = the face-edge each came from.  counts
 *   [3 F] int32 by face-edge: how many selected face-edges have its vertex pair (0 when not selected).  pairs [3 F][2] int32
 *   by sorted position: (face, face) at the first key of a run of exactly two face-edges of two different faces (trimesh's
 *   face_adjacency: group_rows(edges_sorted, require_count=2) minus the pairs within one face), (-1, -1) elsewhere.
 * gsr_regions_components: union-find over the pairs.  parent [F] int32 = the smallest face index of f's component, for every
 *   f (parent[parent[f]] == parent[f]): the hooks point the larger root at the smaller, and the flatten pass that follows
 *   writes each word once, from its own face's thread, after a find that stores nothing; root_flag [F] int32 = 1 for the
 *   selected faces with parent[f] == f.
 * gsr_regions_labels: root_scan = the INCLUSIVE scan of root_flag.  label [F] int32 = root_scan[parent[f]] - 1 -- components
 *   numbered by ascending smallest face, as scipy's connected_components numbers them -- and -1 where not selected; count [F]
 *   int32 (zero before): faces per label.
 * gsr_regions_select: kept_scan = the INCLUSIVE scan over the labels of count > face_threshold.  Region r = kept_scan[l] - 1
 *   of a kept label l: kept_label [cap], kept_count [cap]; region [F] int32 = the face's region or -1.
 * gsr_regions_boxes: boxes [cap][2][3] uint32, per region the minimum and maximum over the three vertices of its faces (verts
 *   [V,3] f32) and over its faces' G points (points [F G,3] f32, face-major), each as the f32's bits b mapped to b | 2^31
 *   (b >= 0) or ~b: unsigned order = float order, -0 counted as +0; a slot no face reached holds 2^32 - 1 (min) / 0 (max).
 * gsr_regions_inside: box: [host] 6 doubles (lo xyz, hi xyz); inside [V] uint8 = lo < (double) v < hi on all three axes.
 * gsr_regions_cut_mark: keep [F] int32 = any (cut_inner = 0) / none (cut_inner = 1) of the face's vertices is inside
 *   (cut_mesh_by_boundingbox, :227-251); referenced [V] int32 = the vertex belongs to a kept face.
 * gsr_regions_cut_emit: with the INCLUSIVE scans of keep and referenced: faces_out [kept,3] int32 in the faces' order with the
 *   vertices renumbered in ascending old index (remove_unreferenced_vertices), face_mask [F] uint8, vert_map [V] int32 (-1:
 *   dropped), old_of_new [referenced] int32.
 * gsr_regions_gather: dst [n_rows][C] = src [old_of_new[row]][C] for 4-byte elements.
 * gsr_regions_boundary: edge_mark [V] uint8 = the vertex lies on a face-edge of count exactly 1; with inside != NULL, face_mark
 *   [V] uint8 = it belongs to a face with some but not all of its vertices inside (:102-109).
 * gsr_regions_label_mask: out [F] uint8 = label[f] >= 0 and count[label[f]] >= min_count. */
int gsr_regions_edge_keys(int F, const int* faces, const unsigned char* mask, const unsigned char* colour, int cut,
                          unsigned char* selected, long long* keys, int* err, gsr_stream_t stream);
int gsr_regions_edge_runs(int F, const long long* sorted_keys, const long long* order, int* counts, int* pairs, gsr_stream_t stream);
int gsr_regions_components(int F, const int* pairs, const unsigned char* selected, int* parent, int* root_flag, gsr_stream_t stream);
int gsr_regions_labels(int F, const int* parent, const int* root_scan, const unsigned char* selected, int* label, int* count,
                       gsr_stream_t stream);
int gsr_regions_select(int F, const int* count, int face_threshold, const int* kept_scan, const int* label, int cap, int* kept_label,
                       int* kept_count, int* region, gsr_stream_t stream);
int gsr_regions_boxes(int F, int G, int V, const int* faces, const float* verts, const float* points, const int* region, int cap,
                      unsigned int* boxes, int* err, gsr_stream_t stream);
int gsr_regions_inside(int V, const float* verts, const double* box, unsigned char* inside, gsr_stream_t stream);
int gsr_regions_cut_mark(int F, int V, const int* faces, const unsigned char* inside, int cut_inner, int* keep, int* referenced,
                         int* err, gsr_stream_t stream);
int gsr_regions_cut_emit(int F, int V, const int* faces, const int* keep, const int* keep_scan, const int* referenced,
                         const int* referenced_scan, int* faces_out, unsigned char* face_mask, int* vert_map, int* old_of_new,
                         gsr_stream_t stream);
int gsr_regions_gather(int n_rows, int C, const int* old_of_new, const void* src, void* dst, gsr_stream_t stream);
int gsr_regions_boundary(int F, int V, const int* faces, const int* counts, const unsigned char* inside, unsigned char* edge_mark,
                         unsigned char* face_mark, int* err, gsr_stream_t stream);
int gsr_regions_label_mask(int F, const int* label, const int* count, int min_count, unsigned char* out, gsr_stream_t stream);

/* ---- The stitch of update_mesh_topo's back half: connect_two_meshes (gaustar_trainers/refined_mesh.py:158-215) with
 * reset_duplicate_vert (:114-123) and merge_vert_around_holes (:126-155), the watertight test (:639) and the face-mask
 * bookkeeping (:205-206, :656-658): gaustar_amd.regions.  fill_holes (:589, :617, :652) and the reference areas (:683-687) are
 * gsr_splice_* below.  Conventions as for gsr_regions_*: device pointers, asynchronous on
 * `stream`, no float atomics, every output an integer or an exactly defined float.  err [1] int32 (zero before): bit 0 = an
 * index outside its array, bit 1 = a coordinate that is NaN or infinite, bit 2 = an index listed twice.
 * gsr_stitch_nn_tile / _nn_queries: the candidates staged in LDS at once and the queries of a workgroup (for the tests).
 * gsr_stitch_nearest: replaces knn_points(K=1) (:166, :175).  queries [Bq,3], candidates [Bc,3] f32, Bc > 0.  In float64
 *   without contraction, dx = (double) q.x - (double) c.x (dy, dz alike), d2 = (dx dx + dy dy) + dz dz; idx [Bq] int32, d2 [Bq]
 *   f64 = the minimum of (d2, index) in lexicographic order: among equal distances the lowest index.  max_bits [1] uint64 = the
 *   bits of the largest d2 written (cleared by the call; the doubles are not negative, so the bits' order is theirs).
 * gsr_stitch_check_list: list [B] int32 must hold different indices in [0, V); mark [V] int32 is scratch.
 * gsr_stitch_snap_groups: reset_duplicate_vert over concat(b1, V1 + b2) after the two snaps (:171, :178, :184-188).  n21 [B2] =
 *   nearest(pc2 -> pc1), n12 [B1] = nearest(pc1 -> pc2 after its snap).  List entry p < B1 sits at pc1[n21[n12[p]]], entry
 *   B1 + j at pc1[n21[j]], and n21 names a position by the lowest pc1 index holding it, so equal positions are equal source
 *   indices.  rep [B1] int32 is scratch (per source the earliest list entry, by integer atomicMin); remap [V1 + V2] int32 =
 *   the identity, but every listed vertex -> the earliest listed vertex at its position.
 * gsr_stitch_mark: faces_out [F,3] = remap[faces] (faces where remap == NULL); keep [F] int32 = mask[f] where mask != NULL, else
 *   the face's three indices differ (nondegenerate_faces, :193, :201, without trimesh's height test); referenced [V] int32 =
 *   the vertex belongs to a kept face.  The scans of keep and referenced go to gsr_regions_cut_emit (update_faces,
 *   remove_unreferenced_vertices, :194-195, :202-203).
 * gsr_stitch_hole_components: merge_vert_around_holes :129-142.  counts [F,3] from gsr_regions_edge_runs.  pairs [3 F][2] int32
 *   = the vertex pair of every face-edge of count != 2, (-1, -1) for the others; hole [V] uint8 = the vertex ends such an
 *   edge; parent [V] int32 = the lowest vertex of its component under those edges; root_flag [V] int32 = 1 at the hole
 *   vertices that are that lowest vertex.
 * gsr_stitch_hole_move: :144-152.  size [V] int32 is scratch (at a lowest vertex, its component's vertices); verts_out [V,3] =
 *   verts, with the hole vertices of components of at most max_hole_vert_num vertices at their lowest vertex's position.
 * gsr_stitch_pos_keys / _pos_heads / _pos_remap: reset_duplicate_vert (:114-123) by true grouping.  list [H] int32: ascending
 *   vertex indices.  key_xy, key_z [H] int64: the coordinates' bits, -0 as +0 (equal numbers, equal keys; their order means
 *   nothing).  order [H] int64: the list entries after stable sorts by key_z, then key_xy.  head [H] int32 = i where sorted
 *   entry i differs in position from entry i - 1 (NaN differs from everything), else 0; first = the running maximum of head.
 *   remap [V] int32 (the identity before): every listed vertex -> the lowest listed vertex of its position.
 * gsr_stitch_compose_mask: out [F] uint8 = outer[f] and inner[outer_scan[f] - 1] (outer_scan: the INCLUSIVE scan of outer):
 *   `m = outer; m[outer] = inner` (:205-206, :656-658).
 * gsr_stitch_vert_map: out [V] int32 = map2[remap2[map1[remap1[v]]]], -1 as soon as map1 says dropped.
 * gsr_stitch_watertight: bad [1] int32 = some face-edge's count is not 2 (cleared by the call; trimesh is_watertight, :639,
 *   also wants F > 0). */
int gsr_stitch_nn_tile(void);
int gsr_stitch_nn_queries(void);
int gsr_stitch_nearest(int Bq, int Bc, const float* queries, const float* candidates, int* idx, double* d2,
                       unsigned long long* max_bits, int* err, gsr_stream_t stream);
int gsr_stitch_check_list(int B, int V, const int* list, int* mark, int* err, gsr_stream_t stream);
int gsr_stitch_snap_groups(int B1, int B2, int V1, int V2, const int* b1, const int* b2, const int* n21, const int* n12, int* rep,
                           int* remap, gsr_stream_t stream);
int gsr_stitch_mark(int F, int V, const int* faces, const int* remap, const unsigned char* mask, int* faces_out, int* keep,
                    int* referenced, int* err, gsr_stream_t stream);
int gsr_stitch_hole_components(int F, int V, const int* faces, const int* counts, int* pairs, unsigned char* hole, int* parent,
                               int* root_flag, int* err, gsr_stream_t stream);
int gsr_stitch_hole_move(int V, int max_hole_vert_num, const unsigned char* hole, const int* parent, int* size, const float* verts,
                         float* verts_out, gsr_stream_t stream);
int gsr_stitch_pos_keys(int H, const int* list, const float* verts, long long* key_xy, long long* key_z, gsr_stream_t stream);
int gsr_stitch_pos_heads(int H, const long long* order, const int* list, const float* verts, int* head, gsr_stream_t stream);
int gsr_stitch_pos_remap(int H, const long long* order, const int* list, const int* first, int* remap, gsr_stream_t stream);
int gsr_stitch_compose_mask(int F, const unsigned char* outer, const int* outer_scan, const unsigned char* inner, int n_inner,
                            unsigned char* out, gsr_stream_t stream);
int gsr_stitch_vert_map(int V, const int* remap1, const int* map1, const int* remap2, const int* map2, int* out, gsr_stream_t stream);
int gsr_stitch_watertight(int F, const int* counts, int* bad, gsr_stream_t stream);

/* ---- The rest of update_mesh_topo (gaustar_trainers/refined_mesh.py:463-693): fill_holes (:589, :617, :652) by a canonical rule
 * of this project, the reference areas (:683-687) and the mean unique-edge length of force_short_edge (:484-485):
 * gaustar_amd.regions.fill_small_holes / update_mesh_topology.  Conventions as for gsr_regions_* and gsr_stitch_*: device
 * pointers, asynchronous on `stream`, no host synchronisation, no float atomics.  err [1] int32 (zero before): bit 0 = a vertex
 * index outside [0, V); such a face is left out.
 * The rule.  Boundary face-edges are those of count exactly 1 (gsr_regions_edge_runs; trimesh's group_rows(edges_sorted,
 *   require_count=1)), each with the direction a -> b it has in its face.  Taken undirected they split the vertices they touch
 *   into components; a component is a rim iff every one of its vertices ends exactly two boundary edges, and is then a simple
 *   cycle.  Rims of 3 or 4 vertices are filled (trimesh's hole_to_faces); every other component is left as it is.  With m the
 *   rim's lowest vertex, x < y its two neighbours on the rim and o the vertex opposite m: a triangle rim gives (m, x, y), a quad
 *   rim A = (m, x, o) and B = (o, y, m) -- the diagonal passes through the lowest vertex.  A new face (a, b, c) is reversed to
 *   (a, c, b) iff the boundary edge between a and b runs a -> b in its own face (trimesh's winding repair, which tests the new
 *   face's first edge only): the triangle and A on m-x, B on o-y, each on its own.  New faces are appended after the existing
 *   ones, rims in ascending m, A before B.  No new face is dropped on geometry.  Departure from trimesh, on purpose: where its
 *   answer depends on networkx's cycle_basis traversal (the diagonal, the order, a component with a vertex of degree != 2, which
 *   it may fill in part) this rule decides; elsewhere the two agree.
 * gsr_splice_workspace_bytes: the bytes of gsr_splice_mean's workspace.
 * gsr_splice_rim_edges: counts [F,3] from gsr_regions_edge_runs.  pairs [3 F][2] int32 = the vertex pair (a, b) of every
 *   face-edge of count 1, (-1, -1) for the others; on_rim [V] uint8 = the vertex ends such an edge; degree [V] int32 = how many
 *   it ends; slots [V][2] uint32 = the first two of them as neighbour << 1 | (the edge leaves this vertex), in no defined order;
 *   parent [V] int32 = the lowest vertex of its component under those edges; root_flag [V] int32 = 1 at the rim vertices that
 *   are that lowest vertex.
 * gsr_splice_rim_census: size, bad [V] int32 are scratch (at a lowest vertex: its component's vertices; some degree != 2);
 *   new_faces [V] int32 = 1 / 2 at the lowest vertex of a rim of 3 / 4 vertices, 0 elsewhere.
 * gsr_splice_rim_emit: new_scan = the INCLUSIVE scan of new_faces, n_new its total.  faces_out [n_new,3] int32 and rim_of_new
 *   [n_new] int32 (the m of each new face), a rim's faces at new_scan[m] - new_faces[m].
 * gsr_splice_face_areas: area [F] f64 = trimesh's area_faces: on doubles converted from the f32 vertices, without contraction,
 *   u = v1 - v0, w = v2 - v1, c = u x w (each component two rounded products and one subtraction), s = (cx cx + cy cy) + cz cz,
 *   area = 0.5 sqrt(s); 0 for a face left out.
 * gsr_splice_edge_lengths: keys [n] int64 = min << 32 | max of a vertex pair (gsr_regions_edge_keys, made unique by the
 *   caller); length [n] f64 = sqrt((dx dx + dy dy) + dz dz) on the widened coordinates.
 * gsr_splice_mean: mean [1] f64 = (the sum of x [n] f64, n > 0) / n by a fixed-order reduction: min(ceil(n / 256), 2048)
 *   workgroups whose threads add their elements in ascending index, a shuffle tree per wave, the waves in order, then one
 *   workgroup's strided sums and tree.  The same bits from call to call. */
size_t gsr_splice_workspace_bytes(void);
int gsr_splice_rim_edges(int F, int V, const int* faces, const int* counts, int* pairs, unsigned char* on_rim, int* degree,
                         unsigned int* slots, int* parent, int* root_flag, int* err, gsr_stream_t stream);
int gsr_splice_rim_census(int V, const int* degree, const int* parent, int* size, int* bad, int* new_faces, gsr_stream_t stream);
int gsr_splice_rim_emit(int V, int n_new, const int* new_faces, const int* new_scan, const unsigned int* slots, int* faces_out,
                        int* rim_of_new, gsr_stream_t stream);
int gsr_splice_face_areas(int F, int V, const int* faces, const float* verts, double* area, int* err, gsr_stream_t stream);
int gsr_splice_edge_lengths(int n, int V, const long long* keys, const float* verts, double* length, int* err, gsr_stream_t stream);
int gsr_splice_mean(long long n, const double* x, void* workspace, double* mean, gsr_stream_t stream);

/* ---- The colours a frame hands to the next one: get_color_mesh (gaustar_scene/sugar_model.py:578-588), the face colours
 * update_mesh_topo carries through connect_two_meshes (gaustar_trainers/refined_mesh.py:183) and the SH dc of a model built from
 * a coloured mesh (sugar_model.py:235-240, :386): gaustar_amd.handover, regions.TopologyUpdate.with_colors,
 * harness.SurfaceGaussians.color_mesh / from_mesh.  Conventions as for gsr_regions_* and gsr_splice_*: device pointers,
 * asynchronous on `stream`, no host synchronisation, no float atomics.  err [1] int32 (zero before): bit 0 = an index outside
 * its array; such an element is left out (its output is zero).  A colour is four bytes r, g, b, a; colour arrays are 4-byte
 * aligned.  Vertex colours are rows of `stride` >= 3 floats of which the first three are r, g, b in [0,1].
 * Two departures from trimesh, on purpose.  (1) The roundings below are this project's statement of trimesh's vertex <-> face
 *   colour conversions; trimesh is not among this project's dependencies, so parity with it is not pinned by a test.  (2) A
 *   face made by fill_small_holes carries (0, 0, 0, 0) and is left out of the vertex means; trimesh's fill_holes gives new
 *   faces a library default colour, which would tint the vertices of every filled rim.
 * gsr_handover_face_colors: sh_dc [F G,3] f32, face-major, G in {1, 3, 4, 6}; rgba [F,4].  Per face and channel, every operation
 *   rounded to f32 and nothing contracted: m = (((x0 + x1) + ...) + x_{G-1}) / G, c = (m C0 + 0.5) 255 with
 *   C0 = 0.28209479177387814 rounded to f32, truncated toward zero and clipped to [0, 255]; alpha 255.  numpy's result for
 *   np.clip(np.int32(SH2RGB(np.average(dc, axis=1)) * 255), 0, 255) wherever the truncation fits an int32; beyond it (and for
 *   NaN, 0) numpy's cast is not defined and this saturates.
 * gsr_handover_vertex_to_face: faces [F,3] int32 over V vertices; rgba [F,4].  Per vertex u8 = clip(rint(255 c), 0, 255), the
 *   product in f32, ties to even (NaN: 0); per face and channel floor((u0 + u1 + u2) / 3); alpha 255.
 * gsr_handover_face_to_vertex: face_rgba [F,4]; sums [V,4] int32, 16-byte aligned, is scratch (cleared here); vert_rgba [V,4].
 *   Per vertex and channel the floor of the integer mean over its incident faces whose alpha is not 0, alpha 255; a vertex with
 *   no such face gets (0, 0, 0, 0).  The sums are 32-bit integer adds, so their order does not show: the same bytes every call.
 * gsr_handover_sh_dc: bary [G,3] f32 (gaustar_amd.harness.BARY_COORDS rounded to f32); sh_dc [F G,3] f32.  Per Gaussian g of a
 *   face (v0, v1, v2) and channel, in f32 without contraction: c = (b_g0 v0 + b_g1 v1) + b_g2 v2, dc = (c - 0.5) / C0, a true
 *   division.
 * gsr_handover_gather: origin [n] int32: k >= 0 = base_rgba [Fb,4] row k; -1 - k = face k of the fusion mesh (fusion_faces
 *   [Ff,3] over Vf vertices, fusion_colors), coloured as gsr_handover_vertex_to_face colours it; INT32_MIN = a filled face,
 *   (0, 0, 0, 0).  rgba [n,4]. */
int gsr_handover_face_colors(int F, int G, const float* sh_dc, unsigned char* rgba, gsr_stream_t stream);
int gsr_handover_vertex_to_face(int F, int V, const int* faces, const float* colors, int stride, unsigned char* rgba, int* err,
                                gsr_stream_t stream);
int gsr_handover_face_to_vertex(int F, int V, const int* faces, const unsigned char* face_rgba, int* sums, unsigned char* vert_rgba,
                                int* err, gsr_stream_t stream);
int gsr_handover_sh_dc(int F, int G, int V, const int* faces, const float* colors, int stride, const float* bary, float* sh_dc,
                       int* err, gsr_stream_t stream);
int gsr_handover_gather(int n, const int* origin, int Fb, const unsigned char* base_rgba, int Ff, int Vf, const int* fusion_faces,
                        const float* fusion_colors, int stride, unsigned char* rgba, int* err, gsr_stream_t stream);

/* ---- Points followed on the surface from frame to frame: tracking_face (gaustar_tools/tracking_util.py:34-148) and the binding
 * step of find_face_of_tags (:20-27): gaustar_amd.tracking.  Conventions as for gsr_stitch_* and gsr_splice_*: device pointers,
 * asynchronous on `stream`, no host synchronisation, no float atomics, no scratch, every output an integer or a float defined
 * operation by operation.  All arithmetic is float64 without contraction: verts [V,3] f64, faces [F,3] int32, ids [K] int32,
 * bary [K,3] f64, pos [K,3] f64.  err [1] int32 (zero before): bit 0 = an id, a rank, a list entry or a face's vertex index
 * outside its array; bit 1 = a vertex or position coordinate that is not finite; bit 3 = a re-bound barycentric that is not
 * >= 0 (the reference's `assert np.all(face_bary >= 0)`, :125: a degenerate nearest face).  An element err speaks of is left out:
 * its float outputs are NaN, its id is unchanged (0 from gsr_track_rebind_displaced).
 * Definitions (tests/tracking_ref.py restates them in numpy).
 *   dot(a,b) = (a.x b.x + a.y b.y) + a.z b.z.
 *   bary_to_point(t0,t1,t2,b): per coordinate (b0 t0 + b1 t1) + b2 t2 -- trimesh's barycentric_to_points,
 *     (triangles * b[:, :, None]).sum(axis=1).
 *   point_to_bary(t0,t1,t2,p), the "cramer" method: e0 = t1 - t0, e1 = t2 - t0, w = p - t0; d00 = dot(e0,e0), d01 = dot(e0,e1),
 *     d02 = dot(e0,w), d11 = dot(e1,e1), d12 = dot(e1,w); inv = 1.0 / (d00 d11 - d01 d01); b2 = (d00 d12 - d01 d02) inv;
 *     b1 = (d11 d02 - d01 d12) inv; b0 = (1 - b1) - b2.  This is the project's statement of trimesh's points_to_barycentric:
 *     trimesh forms its dots through a BLAS product whose order is not defined, and trimesh is not among this project's
 *     dependencies, so parity with it is not pinned by a test.
 *   centre(f) = ((t0 + t1) + t2) / 3.0 per coordinate -- np.average(verts[faces], axis=-2) (:87).
 *   nearest(p): with dx = p.x - centre_j.x (dy, dz alike) and s_j = sqrt((dx dx + dy dy) + dz dz), the lowest j among those
 *     with the smallest s_j -- np.argmin(np.linalg.norm(p - centres, axis=-1)) (:110-112).  The comparison is on the ROUNDED
 *     square root, as numpy's is: two different squared distances can share a square root, and then the lower index wins even
 *     if its squared distance is the larger one.
 * gsr_track_nn_tile / _nn_queries: the centres staged in LDS at once and the queries of a workgroup (for the tests).
 * gsr_track_positions: pos[k] = bary_to_point(verts[faces[ids[k]]], bary[k]) (:70).
 * gsr_track_centres: centres [F,3] f64 = centre(f).
 * gsr_track_rebind_survivors: mask [F0] uint8 = track_face_mask, rank [F0] int32 = its EXCLUSIVE scan (np.sum(mask[:i]), :94),
 *   new mesh of F1 faces over V1 vertices.  For point k with mask[ids[k]]: j = rank[ids[k]], nb = point_to_bary(new face j,
 *   pos[k]); if all three components are >= 0 (NaN fails, as in numpy) ids[k] = j, bary[k] = nb, in place (:102-107).  flag [K]
 *   int32 = 1 for every other point, and for a point whose face did not survive.  stats [3] int32 (cleared by the call):
 *   points kept / moved off their face / lost, by integer atomics.
 * gsr_track_todo: flag_scan = the INCLUSIVE scan of flag.  todo = the flagged k, ascending; n_todo [1] int32 = their number.
 * gsr_track_nearest: idx [slot] int32 = nearest(queries[k]) over centres [F1,3], F1 > 0, for slot < n = min(K, *n_live) (K where
 *   n_live == NULL) and k = list[slot] (slot where list == NULL).  The grid is sized for K; its surplus workgroups exit on
 *   *n_live, so there is no host read between the passes.  A square root per pair (csrc/gsr_track.hip's header says why).
 * gsr_track_rebind_displaced: for slot < n and k as above, j = idx[slot]: ids[k] = j, bary[k] = nb = point_to_bary(new face j,
 *   pos[k]) (:115-117; with list == NULL and clamp == 0 this is find_face_of_tags' :24-27, unclamped as the reference leaves it).
 *   clamp != 0: if any component is < 0, a component < 0 becomes 0 and nb = nb / ((nb0 + nb1) + nb2) (:118-120); a component
 *   that is then still not >= 0 sets err bit 3. */
int gsr_track_nn_tile(void);
int gsr_track_nn_queries(void);
int gsr_track_positions(int K, int F, int V, const int* faces, const double* verts, const int* ids, const double* bary, double* pos,
                        int* err, gsr_stream_t stream);
int gsr_track_centres(int F, int V, const int* faces, const double* verts, double* centres, int* err, gsr_stream_t stream);
int gsr_track_rebind_survivors(int K, int F0, int F1, int V1, const unsigned char* mask, const int* rank, const int* new_faces,
                               const double* new_verts, const double* pos, int* ids, double* bary, int* flag, int* stats, int* err,
                               gsr_stream_t stream);
int gsr_track_todo(int K, const int* flag, const int* flag_scan, int* todo, int* n_todo, gsr_stream_t stream);
int gsr_track_nearest(int K, const int* list, const int* n_live, int F1, const double* queries, const double* centres, int* idx,
                      gsr_stream_t stream);
int gsr_track_rebind_displaced(int K, const int* list, const int* n_live, const int* idx, int F1, int V1, const int* new_faces,
                               const double* new_verts, const double* pos, int* ids, double* bary, int clamp, int* err,
                               gsr_stream_t stream);

/* ---- Scoring a result: the distance from points to a mesh, surface samples, distance statistics, an image pair's squared
 * error: gaustar_amd.evaluate.  It takes the place of the reference's scorer (gaussian_splatting/metrics.py,
 * utils/image_utils.py), which reads PNG directories through torchvision and lpips and has no geometric score; LPIPS is not
 * offered.  Conventions as for gsr_track_*: device pointers, asynchronous on `stream`, no host synchronisation, no float atomics,
 * no scratch; verts [V,3] f64, faces [F,3] int32; all geometry is float64 without contraction, in the order written here.  err
 * [1] int32 (zero before): bit 0 = a face's vertex index or a list entry outside its array; bit 1 = a coordinate that is not
 * finite, or a query for which no face ranks; bit 3 = the sampling weights are not usable (gaustar_amd.evaluate also sets it
 * when no face has a positive, finite area).  tests/eval_ref.py restates all of it in numpy.
 * Definitions.
 *   dot, bary_to_point: as for gsr_track_*.
 *   closest(p; a,b,c), the region test of Ericson, Real-Time Collision Detection, 5.1.5, with one reciprocal and no branch:
 *     ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c;
 *     d1 = dot(ab,ap), d2 = dot(ac,ap), d3 = dot(ab,bp), d4 = dot(ac,bp), d5 = dot(ab,cp), d6 = dot(ac,cp);
 *     vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, e = d4 - d3, g = d5 - d6;
 *     the first that holds gives (nv, nw, den):
 *       A   d1 <= 0 and d2 <= 0               (0, 0, 1)
 *       B   d3 >= 0 and d4 <= d3              (1, 0, 1)
 *       AB  vc <= 0 and d1 >= 0 and d3 <= 0   (d1, 0, d1 - d3)
 *       C   d6 >= 0 and d5 <= d6              (0, 1, 1)
 *       AC  vb <= 0 and d2 >= 0 and d6 <= 0   (0, d2, d2 - d6)
 *       BC  va <= 0 and e >= 0 and g >= 0     (-, e, e + g)
 *       inside, otherwise                     (vb, vc, (va + vb) + vc)
 *     r = 1.0 / den; w = nw r; v = nv r, on BC v = 1.0 - w; u = (1.0 - v) - w, and 0 if that is < 0;
 *     q = a + (ab v + ac w) per coordinate; d = p - q; dist2 = dot(d,d).
 *     A face of repeated or collinear vertices falls into a vertex or an edge region and gives the distance to that point or
 *     segment, except where den is 0 (a == b with p beside them): dist2 is then NaN.  A pair whose dist2 is NaN ranks nothing.
 *   nearest face of p: the lowest j among those with the smallest dist2 -- the lexicographic minimum of (dist2, j).  The
 *     square root is taken once, of the winner's dist2.
 *   area(f): u = t1 - t0, w = t2 - t1, c = u x w (each component two rounded products and one subtraction),
 *     0.5 sqrt((cx cx + cy cy) + cz cz) -- gsr_splice_face_areas' statement on f64 vertices; 0 for a face left out.
 *   sampling weights (formed by the caller in integers): m = max area = mu 2^e with mu in [0.5, 1); w_f = (int64) floor(area_f
 *     2^(32-e)), so max w lies in [2^31, 2^32); cum = the inclusive int64 scan of w.
 *   sample k of n: W = cum[F-1], q = W div n, r = W mod n, t_k = k q + min(k, r) + q div 2; face = the lowest f with cum[f] > t_k
 *     (a face of weight 0 is never taken, the faces are non-decreasing in k).  z = mix(seed + (k + 1) 0x9E3779B97F4A7C15) mod
 *     2^64 with mix(z): z = (z ^ (z >> 30)) 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) 0x94D049BB133111EB; z ^ (z >> 31)
 *     (splitmix64's finaliser).  s = ((z >> 32) + 0.5) 2^-32, t = ((z & 0xffffffff) + 0.5) 2^-32; if s + t > 1: s = 1 - s, t =
 *     1 - t; bary = ((1 - s) - t, s, t): every step exact, the weights >= 0 and of sum exactly 1.  point = bary_to_point.
 *   scores (gaustar_amd.evaluate.mesh_distance, A the result, B the ground truth, n samples of each, d_AB the distances of A's
 *     samples to B): mean = sum d / n, mean of squares = sum d d / n, max; chamfer = mean_AB + mean_BA, chamfer_sq the same of
 *     the means of squares; per threshold tau: precision = #(d_AB < tau) / n, recall = #(d_BA < tau) / n, fscore = 2 P R / (P
 *     + R), 0 where P + R = 0.  mse = SSE / count, psnr = 20 log10(1 / sqrt(mse)) in f64 (the reference takes the mean and the
 *     logarithm in f32).
 * gsr_eval_tile / _queries / _max_thresholds: the faces staged in LDS at once, the queries of a workgroup, the most thresholds
 *   of one gsr_eval_distance_stats call.  gsr_eval_workspace_bytes: the workspace of the two reducing calls.
 * gsr_eval_gather: tri [9,F] f64, row 3 i + k = coordinate k of vertex i of every face; NaN for a face left out.
 * gsr_eval_closest: slot s < n = min(S, *n_live) (S where n_live == NULL) is query k = list[s] (s where list == NULL) of
 *   queries [K,3]; a k outside [0, K) sets err bit 0.  Per slot: face [S] int32 = the nearest face over tri (F > 0), bary [S,3]
 *   = (u, v, w), closest [S,3] = q, dist [S] = sqrt(dist2).  No face ranks: face -1, dist +inf, bary and closest NaN, err bit 1.
 *   The grid is sized for S; its surplus workgroups exit on *n_live.
 * gsr_eval_areas: area [F] f64 = area(f).
 * gsr_eval_sample: cum [F] int64; n > 0 samples: face_ids [n] int32, bary [n,3], points [n,3]; cum[F-1] < n sets err bit 3.
 * gsr_eval_distance_stats: dist [K] f64 >= 0, thresholds [T], T <= 8.  out, 3 + T words of 64 bits (cleared by the call): f64
 *   sum d; f64 sum of (d d); the largest d (non-negative doubles order as their bit patterns: an integer max); then per
 *   threshold the int64 count of d < tau.  The sums by the fixed-order reduction of gsr_splice_mean, the rest by integer atomics:
 *   the same bits from call to call.
 * gsr_eval_image_sse: pred, gt [C,H,W] f32 with element strides; mask [H,W] bytes, contiguous, or NULL (a pixel counts where its
 *   byte is not 0).  Per element p = pred, with clamp01 != 0 p = (pred < 0 ? 0 : pred > 1 ? 1 : pred) (NaN stays NaN, as
 *   torch.clamp leaves it); e = p - gt and e e in f32, as torch computes (a - b) ** 2; the square widened to f64 and summed in
 *   that fixed order.  out, 2 words (cleared by the call): f64 SSE, int64 count of elements. */
int gsr_eval_tile(void);
int gsr_eval_queries(void);
int gsr_eval_max_thresholds(void);
size_t gsr_eval_workspace_bytes(void);
int gsr_eval_gather(int F, int V, const int* faces, const double* verts, double* tri, int* err, gsr_stream_t stream);
int gsr_eval_closest(int S, const int* list, const int* n_live, int K, int F, const double* queries, const double* tri, int* face,
                     double* bary, double* closest, double* dist, int* err, gsr_stream_t stream);
int gsr_eval_areas(int F, int V, const int* faces, const double* verts, double* area, int* err, gsr_stream_t stream);
int gsr_eval_sample(int n, int F, int V, const int* faces, const double* verts, const long long* cum, unsigned long long seed,
                    int* face_ids, double* bary, double* points, int* err, gsr_stream_t stream);
int gsr_eval_distance_stats(long long K, const double* dist, int T, const double* thresholds, void* workspace, void* out,
                            gsr_stream_t stream);
int gsr_eval_image_sse(int C, int H, int W, const float* pred, long long ps0, long long ps1, long long ps2, const float* gt,
                       long long gs0, long long gs1, long long gs2, const unsigned char* mask, int clamp01, void* workspace, void* out,
                       gsr_stream_t stream);

/* ---- Quadric mesh decimation and Laplacian / Taubin smoothing: extract_mesh_fusion's `simplify_face_num` and `smooth`
 * (gaustar_trainers/refined_mesh.py:451-458, Open3D's simplify_quadric_decimation and filter_smooth_laplacian), the Taubin filter
 * of the reference's tools (gaustar_tools/internal_use_tools/fusion_depth.py:80-84) and the decimation that makes a sequence's
 * init_mesh_100k.obj (gaustar_tools/cmr_convert.py:262-266, pyfqmr's simplify_mesh): gaustar_amd.remesh, which states the rules
 * and the departures from those libraries.  This is the project's own round-based parallel statement of Garland-Heckbert
 * decimation; parity with Open3D or pyfqmr is not pinned.  Conventions as for gsr_regions_*: device pointers unless marked
 * [host], asynchronous on `stream`, no host synchronisation, no float atomics; geometry in f64 without contraction, every sum in
 * one stated order.  err [1] int32 (zero before): bit 0 = a face with a vertex index outside [0, V); such a face is not live.
 * All keys are int64, not negative, 2^63 - 1 where there is none.
 * gsr_remesh_setup: verts [V,3] f32, faces [F,3] int32 -> pos [V,3] f64 (widened), live [F] int32 (1 / 0), face_quadric [F,10]
 *   f64 = A p p^T for p = (n / |n|, -(n / |n|) . x0), n = (x1 - x0) x (x2 - x0), A = |n| / 2, as aa ab ac ad bb bc bd cc cd dd;
 *   zeros where |n| is not > 0.
 * gsr_remesh_keys: per live face-edge (a, b), (b, c), (c, a) edge_keys [3 F] = min << 32 | max; per live corner corner_keys
 *   [3 F] = vertex 3F + (3 face + corner); degree [V] int32 (cleared by the call) = the live corners of every vertex.  With the
 *   sorted corner keys and offsets = the exclusive scan of degree [V + 1], vertex v's faces are corners[offsets[v] ..
 *   offsets[v + 1]) in ascending face order (MeshTopology.vertex_face_csr's order): `vf_offsets`, `corners` below.
 * gsr_remesh_vertex_quadrics: quadric [V,10] = the sum of face_quadric over the vertex's list in that order, from 0.
 * gsr_remesh_edge_heads: head [n] int32 = 1 at the first of every run of equal sorted keys (n = 3 live faces: the rest of the
 *   sorted array holds no key).  With head_scan its inclusive scan an edge's id is head_scan - 1 and head_scan[n - 1] the number
 *   of edges (`n_edges` below, read on the device).
 * gsr_remesh_edges: edge_verts [n,2] int32 (u < v), manifold [n] uint8 = exactly two face-edges of two different faces have the
 *   edge; fixed [V] uint8 (the caller's locked mask before) gets 1 at both ends of every edge that is not manifold.
 * gsr_remesh_candidates: key [cap] = f32(cost) bits << 32 | edge id where the edge is a candidate (both ends free, manifold,
 *   link condition, a finite f32 cost, no face turned over or flattened), placement [cap,3] f64 = where the merged vertex goes.
 *   With Q = Q_u + Q_v: Cramer's rule on the 3x3 (cofactors along the first row) where |det| > 1e-10 s^3, s = the largest
 *   |entry|; else the cheapest of P_u, P_v, 0.5 (P_u + P_v), the earlier on ties.  cost = max(x^T Q x, 0).
 * gsr_remesh_select: m1, m2 [V] int64 scratch.  m1[v] = min key over the candidate edges at v; m2[v] = min over ALL edges
 *   (v, w) of min(m1[v], m1[w]); selected [cap] = key where m2[u] == m2[v] == key: no face touches two selected edges.
 * gsr_remesh_cap: [host] n_apply = min(n_selected, (live_faces - target_faces + 1) / 2), 0 where live_faces <= target_faces.
 * gsr_remesh_apply: for every selected edge with key <= *threshold (the n_apply-th smallest selected key): pos[u] = placement,
 *   quadric[u] = quadric[u] + quadric[v], the edge's two faces die, v becomes u in v's other faces.
 * gsr_remesh_apply_attr: attr [V,C] f32, attr[u] = (attr[u] + attr[v]) * 0.5f for the same edges.
 * gsr_remesh_narrow: out [n] f32 = in [n] f64 rounded to nearest.
 * gsr_remesh_smooth: verts [V,3] f32 -> out [V,3] f32 after `steps` sweeps in f64, step s with lambda_even / lambda_odd by the
 *   parity of s (Laplacian: both lambda; Taubin: lambda, mu).  new = prev + lambda (sum w_n prev_n / sum w_n - prev) over the
 *   neighbours in list order, w_n = 1 / (|prev - prev_n| + 1e-12) or, with uniform != 0, 1.  A vertex without neighbours or
 *   with locked[v] (NULL: none) keeps its position.  work_a, work_b [V,3] f64 are scratch. */
int gsr_remesh_setup(int F, int V, const float* verts, const int* faces, double* pos, int* live, double* face_quadric, int* err,
                     gsr_stream_t stream);
int gsr_remesh_keys(int F, int V, const int* faces, const int* live, long long* edge_keys, long long* corner_keys, int* degree,
                    gsr_stream_t stream);
int gsr_remesh_vertex_quadrics(int F, int V, const int* vf_offsets, const long long* corners, const double* face_quadric, double* quadric,
                               gsr_stream_t stream);
int gsr_remesh_edge_heads(int n, const long long* sorted_keys, int* head, gsr_stream_t stream);
int gsr_remesh_edges(int n, int V, const long long* sorted_keys, const long long* order, const int* head_scan, int* edge_verts,
                     unsigned char* manifold, unsigned char* fixed, gsr_stream_t stream);
int gsr_remesh_candidates(int cap, const int* n_edges, int F, int V, const int* edge_verts, const unsigned char* manifold,
                          const unsigned char* fixed, const int* vf_offsets, const long long* corners, const int* faces, const double* pos,
                          const double* quadric, long long* key, double* placement, gsr_stream_t stream);
int gsr_remesh_select(int cap, const int* n_edges, int V, const int* edge_verts, const long long* key, long long* m1, long long* m2,
                      long long* selected, gsr_stream_t stream);
int gsr_remesh_cap(int live_faces, int target_faces, int n_selected, int* n_apply);
int gsr_remesh_apply(int cap, const int* n_edges, int F, int V, const long long* selected, const long long* threshold, const int* edge_verts,
                     const double* placement, const int* vf_offsets, const long long* corners, int* faces, int* live, double* pos,
                     double* quadric, gsr_stream_t stream);
int gsr_remesh_apply_attr(int cap, const int* n_edges, int V, int C, const long long* selected, const long long* threshold,
                          const int* edge_verts, float* attr, gsr_stream_t stream);
int gsr_remesh_narrow(long long n, const double* in, float* out, gsr_stream_t stream);
int gsr_remesh_smooth(int V, const int* nbr_offsets, const int* nbr, const unsigned char* locked, int steps, double lambda_even,
                      double lambda_odd, int uniform, const float* verts, double* work_a, double* work_b, float* out, gsr_stream_t stream);

/* ---- Exact K-nearest-neighbour search of f32 points (pytorch3d's knn_points as gaustar_scene/sugar_model.py:49, :253, :862,
 * :877, :1014 and gaustar_tools/warp_mesh.py:199-213 call it; simple-knn's distCUDA2, simple_knn.cu:147-183) and what the
 * callers make of the rows: gaustar_amd.knn.  The rules, restated in tests/knn_ref.py: queries [N,3] and candidates [M,3] are
 * f32; with d = query - candidate, d2 = (dx dx + dy dy) + dz dz in f32 without contraction; a row holds the K smallest pairs in
 * ascending (d2, candidate index) order, the lower index first among equals; 1 <= K <= gsr_knn_max_k() = 32; slots beyond the
 * number of eligible candidates hold idx = -1, d2 = +inf; a point with a non-finite coordinate is never returned as a
 * neighbour and has, as a query, an empty row; with exclude_self (N == M: the queries are the candidates) candidate j == i is
 * skipped for query i, a duplicate of it at another index is not (boxMeanDist, simple_knn.cu:158, :177).  The result is the
 * exhaustive search's bit for bit: it does not depend on the two orders below, on the tiles or on the call.  All device
 * pointers; every call is asynchronous on `stream`, none synchronises the host, none uses float atomics.
 * gsr_knn_tile / _seed / _queries: T = candidates per tile, S = the seed looks at the 2 S + 1 sorted candidates around a
 *   query's position, Q = queries per (one-wave) workgroup.
 * gsr_knn_workspace_bytes(N, M, K): the candidates' copy, padded to whole tiles, and the tile boxes (N and K do not enter: the
 *   lists are registers); 16-byte aligned.
 * gsr_knn_prepare: order [M] int64 = a permutation of the candidates along a space-filling curve, non-finite ones last (a
 *   30-bit Morton code over the finite candidates' box, gaustar_amd/knn.py; it only orders the work).  Writes the workspace:
 *   the candidates in that order as float4 (xyz, the index as bits; NaN for a non-finite one) and, per tile of T consecutive
 *   ones, the box of its finite points.
 * gsr_knn_search: query_order [N] int64 = a permutation of the queries along the same curve; workgroup w takes the Q queries
 *   query_order[w Q ..].  query_pos [N] int64, by sorted query: where the query would stand among the sorted candidates (its
 *   own position when the queries are the candidates); read only with cull != 0.  cull != 0: per query the K best of the
 *   candidates at sorted positions [pos - S, pos + S] give tau, an upper bound of its K-th distance; a tile is skipped iff the
 *   lower bound of its box -- d2's operations in d2's order, 0 for an axis inside the box -- is > the current bound min(tau, the
 *   list's K-th) of every query of the workgroup.  cull == 0: every tile is visited and there is no seed: the exhaustive mode.
 *   idx [N,K] int32 and d2 [N,K] f32 in the caller's query order.  stats: NULL, or 2 uint64 cleared by the call: pairs
 *   evaluated (seed windows included; N M with cull == 0) and tiles skipped, one integer atomic per workgroup and counter.
 *   M == 0 leaves every row empty; N == 0 is a no-op.
 * gsr_knn_mean_d2: out [N] f32 = ((r0 + r1) + r2) / 3.0f over the first three slots of every row of d2 [N,K], K >= 3, the
 *   expression of simple_knn.cu:182; an empty slot counts as FLT_MAX, the reference's initial `best`, so fewer than three
 *   neighbours give inf (one missing: FLT_MAX / 3 after rounding).
 * gsr_knn_segment_mean: segment_ids [n] int64 ascending, dense in [0, S); order [n] int64 = the element each sorted position
 *   came from; values [n,C] double by element.  out [S,C] double = per run of equal ids the sum over the run in sorted order,
 *   from 0, divided by its length; count [S] int32 = the length (a voxel's mean, gsr_topo_voxel_interp's rule; no atomics).
 * gsr_knn_weighted_mean: interpolate_in_voxel's average (warp_mesh.py:204-211) over the rows idx, d2 [N,K] of a search among M
 *   candidates with values [M,C] double: w_k = exp(-(double) d2_k inv_scale) + 1e-8, out [N,C] double = (sum_k v[idx_k] w_k) /
 *   (sum_k w_k), both sums from 0 for k ascending.  An empty slot counts as (index 0, distance 0), as pytorch3d pads its rows.
 *   The weights are double (the reference's are f32, numpy's exp of an f32 array); exp is evaluated from IEEE operations in a
 *   fixed order (tests/knn_ref.py::exp_neg, within 2 ulp), so the result is reproducible to the bit on any machine. */
int gsr_knn_tile(void);
int gsr_knn_seed(void);
int gsr_knn_queries(void);
int gsr_knn_max_k(void);
size_t gsr_knn_workspace_bytes(int N, int M, int K);
int gsr_knn_prepare(int M, const float* candidates, const long long* order, void* workspace, gsr_stream_t stream);
int gsr_knn_search(int N, int M, int K, const float* queries, const long long* query_order, const long long* query_pos,
                   const void* workspace, int exclude_self, int cull, int* idx, float* d2, unsigned long long* stats,
                   gsr_stream_t stream);
int gsr_knn_mean_d2(int N, int K, const float* d2, float* out, gsr_stream_t stream);
int gsr_knn_segment_mean(int n, int S, int C, const long long* segment_ids, const long long* order, const double* values,
                         double* out, int* count, gsr_stream_t stream);
int gsr_knn_weighted_mean(int N, int K, int C, int M, const int* idx, const float* d2, const double* values, double inv_scale,
                          double* out, gsr_stream_t stream);

/* ---- The Gaussians' density field: SuGaR's compute_density (gaustar_scene/sugar_model.py:1017-1040) with the inverse scaled
 * rotation of get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True) (:619-625) folded in, over the
 * neighbours get_gaussians_closest_to_samples (:1007-1015) finds: gaustar_amd.density, and through it postprocess_mesh
 * (gaustar_trainers/refined_mesh.py:1180-1182).  The inputs are f32; every term is formed in float64 without contraction, in
 * the order below (tests/density_ref.py restates it), and rounded to f32 once at the end.  All device pointers; every call is
 * asynchronous on `stream`, none synchronises the host, none uses float atomics, LDS or scratch, and a result is the same bits
 * in every call.
 * gsr_density_queries_per_wave / _per_workgroup: 16 lanes serve a query, so 4 queries share a wave64 and 16 a workgroup.
 * gsr_density_pack: replaces the three gathers of :1024-1028 by one record.  points [P,3], scaling [P,3] (activated, as
 *   SuGaR.scaling), quaternions [P,4] (real part first, any norm), strengths [P] -> records: P x 48 bytes, three float4
 *   {cx, cy, cz, strength}, {qr, qi, qj, qk}, {s0, s1, s2, 0}, the inputs' bits verbatim.  Every array 16-byte aligned (the
 *   kernel moves 16 bytes at a time).  P == 0 is a no-op.
 * gsr_density_eval: replaces :1031-1035.  x [Q,3] f32, idx [Q,K] int32 with 1 <= K <= 32 and -1 in an empty slot (gsr_knn_search's
 *   rows).  Per slot with Gaussian (c, q, s, strength):
 *     d = (double) x - (double) c;  two_s = 2 / (((qr qr + qi qi) + qj qj) + qk qk);  R = pytorch3d's quaternion_to_matrix:
 *     R00 = 1 - two_s (qj qj + qk qk), R01 = two_s (qi qj - qk qr), R02 = two_s (qi qk + qj qr), R10 = two_s (qi qj + qk qr),
 *     R11 = 1 - two_s (qi qi + qk qk), R12 = two_s (qj qk - qi qr), R20 = two_s (qi qk - qj qr), R21 = two_s (qj qk + qi qr),
 *     R22 = 1 - two_s (qi qi + qj qj);  inv_a = 1 / (s_a < 1e-8 ? 1e-8 : s_a);
 *     w_a = inv_a ((R[0][a] d0 + R[1][a] d1) + R[2][a] d2), a = 0, 1, 2  (:1032's (R diag(inv))^T d);
 *     m = (w0 w0 + w1 w1) + w2 w2, then m < 0 ? 0 : (m > 1e8 ? 1e8 : m)  (:1033's clamp; a NaN stays);
 *     t = ((double) density_factor (double) strength) exp(-0.5 m)  (:1034).
 *   An empty slot, and a slot from K up to 31, has t = +0.0.  u_j = t_j + t_{j+16} for j = 0..15; then four rounds r = 1, 2, 4, 8
 *   of u_j <- u_j + u_{j xor r} over all j at once: a balanced tree, the same in every j.  density [Q] f32 = (float) u_0;
 *   neighbor_opacities: NULL, or [Q,K] f32 = (float) t (the second value of return_closest_gaussian_opacities, :1038).
 *   err: one int32, zero before; bit 0 is set when an index lies outside [-1, P), and that slot counts as empty.  Refused
 *   before any device work: K outside 1..32, P < 1 or a null pointer with Q > 0.  Q == 0 is a no-op. */
int gsr_density_queries_per_wave(void);
int gsr_density_queries_per_workgroup(void);
int gsr_density_pack(int P, const float* points, const float* scaling, const float* quaternions, const float* strengths, void* records,
                     gsr_stream_t stream);
int gsr_density_eval(int Q, int P, int K, const float* x, const int* idx, const void* records, float density_factor, float* density,
                     float* neighbor_opacities, int* err, gsr_stream_t stream);

/* ---- Editing a tracked sequence: the per-Gaussian passes of gaustar_tools/internal_use_tools/gstar_edit.py (cut_gstar :74-119,
 * merge_gstar :122-184, edit_gs_color :295-388, best_fit_transform :28-71), which the reference runs on the host in numpy,
 * trimesh and cv2: gaustar_amd.edit.  tests/edit_ref.py restates every rule below in numpy.  All device pointers unless marked
 * [host]; every call is asynchronous on `stream`, none synchronises the host, none uses float atomics or scratch.  err: the
 * mesh kernels' word (csrc/gsr_mesh.h), ORed into: bit 0 = a vertex or face index outside its array; the calls that index
 * nothing (fit_sums, transform_points, rotate_sh) take it and leave it alone (it may be NULL there).
 * gsr_edit_fit_sums: replaces :48-54 for T frames at once.  src [K,3], dst [T,K,3] f64 (a [K,3] dst is T = 1).  Anchor k counts
 *   in frame t iff its six coordinates src[k], dst[t,k] are finite (a lost point is a NaN row of face_trajectory).  out [T,16]
 *   f64 = {n, abar (3), bbar (3), H row-major (9)}: n the anchors that count, abar = (sum a) / n, bbar = (sum b) / n, H[i][j] =
 *   sum (a_i - abar_i)(b_j - bbar_j), every term one rounded product of two rounded differences.  Two element passes
 *   (centroids, then H about them) and a finish, each one launch over all frames; the sums are taken per workgroup and then
 *   over the workgroups in a fixed order (csrc/gsr_reduce.h), so two calls give the same bits; against the exactly rounded sum
 *   of the same terms a sum of m terms is within m 2^-53 sum |term|.  n == 0 gives NaN centroids and H = 0.  :55-64 (the SVD
 *   of H, the reflection fix, t = bbar - R abar) are the host's: gaustar_amd.edit.fit_rigid.  workspace: T <= 65535 frames,
 *   gsr_edit_fit_workspace_bytes(T, K) bytes.  T == 0 is a no-op; K == 0 is refused.
 * gsr_edit_transform_points: replaces :146 (`np.matmul(R, v) + t`).  x: n rows of `stride` floats; columns [offset, offset + 3)
 *   of every row become, in place and per coordinate i, (float) (((R[i][0] x + R[i][1] y) + R[i][2] z) + t[i]) in float64 from
 *   the f32 inputs: three rounded products, three rounded sums, one rounding to f32.  R [host] 9 doubles row-major; t [host] 3
 *   doubles, or NULL: the last sum is left out (a direction: `_delta_t`, the vector part of `_delta_r`).
 * gsr_edit_rotate_sh: no counterpart (the reference turns an attached object, :146, and leaves its world-frame SH coefficients
 *   as they were).  rest_in, rest_out [N, M - 1, 3] f32, 16-byte aligned, M = 4, 9 or 16; D [M,M] f64 row-major, block diagonal
 *   with blocks of 1, 3, 5, 7 (gaustar_amd.edit.sh_rotation_matrices).  Per Gaussian, channel c and coefficient i of band l
 *   (o = l l <= i < o + 2 l + 1): s = D[i][o] x[o], then s = s + D[i][k] x[k] for k = o + 1 .. o + 2 l ascending, x[k] =
 *   (double) rest_in[n][k - 1][c]; rest_out[n][i - 1][c] = (float) s.  rest_out may be rest_in.
 * gsr_edit_faces_in_halfspaces: replaces :81-102, the planes as data.  verts [V,3] f32, faces [F,3] int32; n_groups <= 16
 *   groups of group_sizes[g] >= 1 planes [host], 64 planes (a, b, c, d) in all, planes [host] [sum,4] f64 in group order.  A
 *   face's centre is per coordinate ((v0 + v1) + v2) / 3.0 in float64 (:82); mask [F] uint8 = 1 iff for some group every plane
 *   of it has ((a cx + b cy) + c cz) + d > 0, strictly.  A face with an index outside [0, V) gets 0 and sets err.
 * gsr_edit_gather_rows: replaces :114-116 (`state_dict[key][gs_mask]`) for all keys in one launch.  kept [n_faces] int32 = the
 *   old face of every new face, each in [0, F).  n_tables <= 8 arrays of 32-bit words: src[e] [F G, row_words[e]], dst[e]
 *   [n_faces G, row_words[e]] (src, dst, row_words: [host] arrays of n_tables entries); rows [G j, G j + G) of dst[e] are rows
 *   [G kept[j], ...) of src[e].  An entry of kept outside [0, F) gives zeros and sets err.
 * gsr_edit_paint: replaces :316-385.  The model: N = F G Gaussians, verts [V,3] f32, faces [F,3] int32, bary [G,3] f32; Gaussian
 *   n = G f + g sits at p = (b_g0 v0 + b_g1 v1) + b_g2 v2 per coordinate, float64 from the f32 inputs (:320-322, there f32).
 *   tri [n_tri,15] f64, n_tri <= 64: per triangle its corners t0, t1, t2 and their (u, v).  The triangles are walked in order
 *   (a Gaussian inside two of them is treated twice, :354); per triangle: bary = point_to_bary(t0, t1, t2, p) (gsr_track's
 *   rule, :358); nrm = -cross(t1 - t0, t2 - t1) / sqrt((x x + y y) + z z), dist = dot(t0 - p, nrm) (:284-292); inside iff every
 *   bary >= -bary_slack and -max_dist < dist < max_dist (:359-362).  An inside Gaussian: with shrink != 0 both of its scales
 *   become shrink_scale (:364); (u, v) = bary_to_point of the corners' (u, v); row = trunc(u h), col = trunc(v w), toward zero
 *   (:369); a texel outside the texture [h,w,C] uint8 (r, g, b order) counts in n_outside and leaves the colour alone.  mode 0,
 *   multiply (:379): rgb = rgb (float) (tex[row][col][0] / 255.0); mode 1, replace (:373-376), C = 3 or 4: where C == 3 or
 *   tex[row][col][3] > alpha_min, rgb = (float) (tex[row][col][0..2] / 255.0).  rgb = dc C0 + 0.5f is formed by the first
 *   triangle that paints and carried through the later ones; at the end dc = (rgb - 0.5f) / C0 (:334, :384), in f32 without
 *   contraction.  scales [N,2], sh_dc [N,3] in place; a Gaussian that was not painted keeps its dc bits, one that was in no
 *   triangle its scales.  stats [2 + n_tri] int32, cleared by the call: the Gaussians painted, the (Gaussian, triangle) pairs
 *   whose texel fell outside, the Gaussians inside each triangle.  A face index outside sets err and leaves the Gaussian out. */
size_t gsr_edit_fit_workspace_bytes(int T, int K);
int gsr_edit_fit_sums(int T, int K, const double* src, const double* dst, void* workspace, double* out, int* err, gsr_stream_t stream);
int gsr_edit_transform_points(long long n, int stride, int offset, float* x, const double* R, const double* t, int* err,
                              gsr_stream_t stream);
int gsr_edit_rotate_sh(int N, int M, const double* D, const float* rest_in, float* rest_out, int* err, gsr_stream_t stream);
int gsr_edit_faces_in_halfspaces(int F, int V, const int* faces, const float* verts, int n_groups, const int* group_sizes,
                                 const double* planes, unsigned char* mask, int* err, gsr_stream_t stream);
int gsr_edit_gather_rows(int n_faces, int F, const int* kept, int G, int n_tables, const void* const* src, void* const* dst,
                         const int* row_words, int* err, gsr_stream_t stream);
int gsr_edit_paint(int N, int G, int F, int V, const int* faces, const float* verts, const float* bary, int n_tri, const double* tri,
                   int h, int w, int C, const unsigned char* texture, int mode, double bary_slack, double max_dist, int shrink,
                   float shrink_scale, int alpha_min, float* scales, float* sh_dc, int* stats, int* err, gsr_stream_t stream);

/* ---- Shape from silhouettes: the visual hull of the rig's alpha masks as a volume of the TSDF fusion above, so that
 * gsr_fusion_count / gsr_fusion_emit extract its mesh: gaustar_amd.hull.  The reference takes the per-frame meshes its depth
 * maps and masks are rendered from out of HumanRF (README.md:38-39); this replaces that source, not a function of the reference.
 * All device pointers unless marked [host]; every call is asynchronous on `stream`, none synchronises the host, none uses
 * atomics: every output is a pure function of the inputs, and the carve state does not depend on the cameras' order or on how
 * they are split into calls.  tests/hull_ref.py restates the rules.
 * gsr_hull_mask_distance: mask [H,W] uint8, H, W >= 2, H <= 65535; a pixel is inside iff mask >= threshold (0..256); 1 <= radius
 *   <= 127.  d2 [H,W] int16: for an inside pixel +min(radius^2, the squared distance to the nearest outside pixel of the image),
 *   for an outside pixel -min(radius^2, the squared distance to the nearest inside pixel); what lies beyond the border is
 *   neither, so an image of one kind holds +-radius^2 throughout, and no entry is 0.  Exact (integers).  workspace:
 *   gsr_hull_mask_distance_workspace_bytes(H, W) bytes.
 * gsr_hull_carve: field [voxels] f32 (+inf before the first camera) and count [voxels] int32 (0 before), 16-byte aligned, over
 *   the fusion's `grid` with the fusion's voxel centres.  cameras: n_cameras records of gsr_hull_camera_bytes() = 144 bytes: 9
 *   doubles R (row-major) and 3 doubles t of the COLMAP world-to-camera transform, fx, fy, cx, cy (doubles; pixel centres at
 *   integer coordinates), the device pointer of the camera's d2 map, int H, int W.  cameras_host: [host] the same bytes, which
 *   are checked (finite, fx, fy > 0, H, W >= 2, d2 not null) before the launch reads its device copy.  Per voxel centre p and
 *   camera, in double without contraction:
 *     q = ((R_r0 p.x + R_r1 p.y) + R_r2 p.z) + t_r per row r; nothing happens unless q.z > 0.01;
 *     u = fx (q.x / q.z) + cx, v = fy (q.y / q.z) + cy; nothing happens unless 0 <= u <= W - 1 and 0 <= v <= H - 1;
 *     x0 = min(floor(u), W - 2), y0 = min(floor(v), H - 2), a = u - x0, b = v - y0;
 *     phi(e) = sign(e) (sqrt(|e|) - 0.5) of the entries at (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1);
 *     top = phi00 + a (phi01 - phi00), bot = phi10 + a (phi11 - phi10), phi = top + b (bot - top);
 *     d = (phi q.z) (2 / (fx + fy)); field = min(field, (float) d); count += 1.
 * gsr_hull_finish: min_views >= 1.  weight = 1 where count >= min_views, else 0; tsdf = (float) clamp(-(double) field /
 *   sdf_trunc, -1, 1) under weight 1, else 0 (negative inside, as gsr_fusion_count reads it); touched [units] uint8 = 1 iff the
 *   unit holds a voxel with weight 1 and |tsdf| < 1.  The fusion's color planes are not written. */
size_t gsr_hull_mask_distance_workspace_bytes(int H, int W);
int gsr_hull_mask_distance(int H, int W, const unsigned char* mask, int threshold, int radius, void* workspace, short* d2,
                           gsr_stream_t stream);
int gsr_hull_camera_bytes(void);
int gsr_hull_carve(int n_cameras, const void* cameras_host, const void* cameras, double voxel_size, const int* grid, float* field,
                   int* count, gsr_stream_t stream);
int gsr_hull_finish(const int* grid, const float* field, const int* count, int min_views, double sdf_trunc, float* tsdf, float* weight,
                    unsigned char* touched, gsr_stream_t stream);

/* ---- Plane-sweep stereo behind a depth prior: the photo-consistency refinement of the visual hull above, which closes over
 * every concavity: gaustar_amd.stereo.  The reference has no counterpart (its depth comes from HumanRF meshes, README.md:38-39).
 * All device pointers unless marked [host]; every call is asynchronous on `stream`, none synchronises the host, none uses
 * atomics; all arithmetic is double without contraction in the order written here, and every output is a pure function of the
 * inputs.  tests/stereo_ref.py restates the rules.  Pixel (row r, column c) has its centre at (x, y) = (c, r); znear = 0.01.
 * gsr_stereo_luma: rgb [H,W,3] uint8 -> luma [H,W] uint8, Y = (77 R + 150 G + 29 B + 128) >> 8.
 * Camera tables: n_sources (1..8) records of gsr_stereo_camera_bytes() = 152 bytes: 9 doubles R_sr (row-major) and 3 doubles
 *   t_sr, the source's pose RELATIVE to the reference camera (R_sr = R_s R_r^T, t_sr = t_s - R_sr t_r, each element three
 *   products added as (a + b) + c, made on the host); the source's fx, fy, cx, cy (doubles); the device pointer of its image
 *   (sweep: luma [H,W] uint8; consistency: refined depth [H,W] f32); the device pointer of its state [H,W] uint8 from the sweep
 *   (consistency only); int H, int W.  sources_host: [host] the same bytes, checked (finite, fx, fy > 0, H, W >= 2, pointers)
 *   before the launch reads the device copy.  ref_cam: [host] the reference camera's fx, fy, cx, cy.
 * gsr_stereo_sweep: params [host] = step, near, far, background, min_var, min_score; step > 0, near, far >= 0, (near + far) /
 *   step <= 4096, (background + far) / step < 32768, min_var > 0; radius R in {1, 2, 3}, N = (2 R + 1)^2; 1 <= min_sources, keep
 *   <= n_sources.  Planes are global per reference camera: z_k = k step, k >= k_min = floor(znear / step) + 1.
 *   A pixel is covered iff its prior d (f32 widened) has znear < d < background; its band is k_lo = max(k_min, ceil((d - near) /
 *   step)) .. k_hi = floor((d + far) / step).
 *   Warp of reference pixel (r, c) on plane k into source s: L = (((c - cx) / fx) z, ((r - cy) / fy) z, z), z = k step; local =
 *   ((R_i0 L.x + R_i1 L.y) + R_i2 L.z) + t_i per row; invalid unless local.z > znear; px = fx_s (local.x / local.z) + cx_s, py
 *   alike; valid iff 0 <= px < W_s - 1 and 0 <= py < H_s - 1 (so x0 = floor(px) <= W_s - 2); ax = px - x0, ay = py - y0; w =
 *   (1 - ay) ((1 - ax) I00 + ax I01) + ay ((1 - ax) I10 + ax I11) on luma widened to double.
 *   Score of (pixel, k, s) over the (2 R + 1)^2 window: every tap on the reference image and every tap's warp on the CENTRE's
 *   plane valid, else invalid.  A = sum g, B = sum g^2 (integers), Vr = N B - A^2; invalid if (double) Vr < (double) (N N)
 *   min_var.  Sw, Sww, Swg: from 0.0, one tap after the other, rows outer, columns inner, left to right (Sww += w w, Swg += w g).
 *   Vs = N Sww - Sw Sw; invalid unless Vs >= N N min_var.  score = (N Swg - Sw A) / sqrt(Vs Vr).
 *   Cost of (pixel, k): v valid sources; unusable if v < min_sources; else T = min(keep, v) and cost = (the T highest scores
 *   added in descending order) / T.
 *   Pick: k* = the usable plane of the band with the highest cost, ties to the smaller k.  state [H,W] uint8: 0 not covered, 1
 *   covered without a usable plane, 2 best cost < min_score, 3 accepted.  If k* - 1 and k* + 1 are in the band and usable: den =
 *   (c- - 2 c0) + c+; if den < 0, delta = clamp((0.5 (c- - c+)) / den, -0.5, 0.5); else delta = 0.
 *   depth [H,W] f32 = (float) ((k* + delta) step) at state 3, the prior's bits elsewhere; score [H,W] f32 = the best cost at
 *   states 2 and 3, else -2; plane [H,W] int16 = k* at states 2 and 3, else -1.
 * gsr_stereo_consistency: for a pixel of state 3 with refined depth z: L as above, local per source; the source agrees iff
 *   local.z > znear, the pixel (int) (px + 0.5), (int) (py + 0.5) (truncation; valid iff inside the image) has sweep state >= 3
 *   and |depth_s - local.z| <= tol there.  state_out = 4 iff at least min_consistent sources agree, else the input state.
 * gsr_stereo_merge: two volumes over one fusion `grid`, arrays 16-byte aligned: tsdf = (w_s >= min_weight and w_h == 1 and t_s >
 *   t_h) ? t_s : t_h (the hull bounds the surface from outside: stereo only carves); weight = w_h; color [3][voxels] = the stereo
 *   volume's where w_s > 0, else 0; touched [units] = 1 iff the unit holds a voxel with weight 1 and |tsdf| < 1. */
int gsr_stereo_camera_bytes(void);
int gsr_stereo_luma(int H, int W, const unsigned char* rgb, unsigned char* luma, gsr_stream_t stream);
int gsr_stereo_sweep(int H, int W, const unsigned char* luma, const float* prior, const double* ref_cam, int n_sources,
                     const void* sources_host, const void* sources, const double* params, int radius, int min_sources, int keep,
                     float* depth, float* score, unsigned char* state, short* plane, gsr_stream_t stream);
int gsr_stereo_consistency(int H, int W, const float* depth, const unsigned char* state, const double* ref_cam, int n_sources,
                           const void* sources_host, const void* sources, double tol, int min_consistent, unsigned char* state_out,
                           gsr_stream_t stream);
int gsr_stereo_merge(const int* grid, const float* tsdf_h, const float* weight_h, const float* tsdf_s, const float* weight_s,
                     const float* color_s, double min_weight, float* tsdf, float* weight, float* color, unsigned char* touched,
                     gsr_stream_t stream);

/* ---- RAFT optical flow, the basic model's inference: gaustar_amd.flow. Replaces data_process/RAFT (demo_GauSTAR.py and the
 * core/ modules it runs).  All activations are f32, NHWC, on the device; every call is asynchronous on `stream`, none
 * synchronises the host, none uses atomics, and every output is a pure function of the inputs with a fixed order of
 * operations.  tests/flow_ref.py restates the model.
 * gsr_flow_slice [host]: `channels` channels of a buffer of `stride` floats per pixel, starting at channel `offset`; the
 *   reference's torch.cat's are slices of one buffer.
 * gsr_flow_prep_image (demo_GauSTAR.py:30-40 load_image, utils/utils.py:7-19 InputPadder 'sintel', raft.py:89-90): image [h,w,3]
 *   uint8, factor 1, 2 or 4 dividing h and w -> out [Hp,Wp,3]: the factor x factor box mean rounded half to even (cv2's
 *   INTER_AREA with cvRound), hs = h / factor, Hp = hs rounded up to a multiple of 8, replicate padding with (Hp - hs) / 2
 *   rows before and the rest after (columns alike), then 2 (x / 255) - 1.
 * gsr_flow_conv (torch.nn.Conv2d as extractor.py and update.py use it): desc [host].  Input: the concatenation of n_in slices
 *   over N images of H x W; kernel 1x1, 3x3, 7x7, 1x5 or 5x1 with zero padding KH / 2, KW / 2; stride 1 or 2; 2 <= Cin <= 384,
 *   2 <= Cout <= 576.  weights: [gsr_flow_packed_k(KH KW Cin)][gsr_flow_packed_n(Cout)] (K rounded up to 16; Cout rounded up to
 *   64, or 4 columns for Cout <= 4) with row (ky KW + kx) Cin + ci, zeros
 *   in the padding, 16-byte aligned.  Per output: the k-ordered f32 fma chain from 0 (v_mfma_f32_32x32x2_f32; for Cout <= 4 the
 *   chains of k = 4 l .. 4 l + 3 (mod 256) for l = 0 .. 63, joined by a fixed tree: one wave per output pixel), + bias, then
 *   x scale + shift where scale is given (eval-mode batch norm, extractor.py:22-26), then act (0 none, 1 relu, 2 sigmoid, 3
 *   tanh), then + residual where residual.base is given, then relu if residual_relu (extractor.py:56); stored to the slice
 *   `out`.  residual may be `out` itself (the flow's update, raft.py:131).
 * gsr_flow_pack_features / gsr_flow_corr_volume (corr.py:52-60 CorrBlock.corr): fmap [P][C] -> packed [C][P rounded up to 64];
 *   volume [P1][P2] = (fmap1 . fmap2) / sqrt(C) with the convolution's chain over c; C a power of four (the scale is exact).
 * gsr_flow_corr_pool (corr.py:25-27): in [rows][h][w] -> out [rows][h/2][w/2], (((a + b) + c) + d) / 4.
 * gsr_flow_corr_lookup (corr.py:29-50, utils/utils.py:57-71 bilinear_sampler): for feature pixel (x, y) of the h8 x w8 grid
 *   with flow (fx, fy), level l of dims (h2, w2) >> l and 0 <= i, j < 9: out[pixel][81 l + 9 i + j] = the bilinear sample of the
 *   pixel's level-l map at ((x + fx) / 2^l + i - 4, (y + fy) / 2^l + j - 4), taps outside the map counting 0.
 * gsr_flow_instance_norm (torch.nn.InstanceNorm2d, extractor.py:28-32, :50-56): x [N][HW][C] -> (x - mean) / sqrt(var + 1e-5)
 *   per (image, channel), biased variance, sums in f64 in a fixed order; then relu if `relu`; then relu(residual + .) where
 *   residual is given.  out may be x.
 * gsr_flow_gru_combine (update.py:50-51, :57-58): mode 0: out = gate h; mode 1: out = (1 - gate) h + gate q; slices of
 *   4-aligned channels; out may be h.
 * gsr_flow_upsample (raft.py:72-83 upsample_flow, utils/utils.py:21-24 unpad, demo_GauSTAR.py:99): mask [h8 w8][576] the mask
 *   head's output; out [h,w,2] in (x, y) order: pixel (Y, X) lies at (Y + pad_top, X + pad_left) of the padded image, in cell
 *   (y, x) at (i, j); weights = softmax_k(0.25 mask[64 k + 8 i + j]), out = sum_k w_k 8 flow(y + k / 3 - 1, x + k % 3 - 1),
 *   cells outside the grid counting 0. */
typedef struct gsr_flow_slice {
    const float* base;
    long long stride;
    int offset, channels;
} gsr_flow_slice;
typedef struct gsr_flow_conv_desc {
    int N, H, W, KH, KW, stride, n_in, Cout, act, residual_relu;
    gsr_flow_slice in[3];
    gsr_flow_slice out, residual;
    const float *weights, *bias, *scale, *shift;
} gsr_flow_conv_desc;
int gsr_flow_packed_k(int K);
int gsr_flow_packed_n(int Cout);
int gsr_flow_prep_image(int h, int w, const unsigned char* image, int factor, float* out, gsr_stream_t stream);
int gsr_flow_conv(const gsr_flow_conv_desc* desc, gsr_stream_t stream);
int gsr_flow_pack_features(int P, int C, const float* fmap, float* packed, gsr_stream_t stream);
int gsr_flow_corr_volume(int P1, int P2, int C, const float* fmap1, const float* packed2, float* volume, gsr_stream_t stream);
int gsr_flow_corr_pool(long long rows, int h, int w, const float* in, float* out, gsr_stream_t stream);
int gsr_flow_corr_lookup(int h8, int w8, int h2, int w2, const gsr_flow_slice* flow, const float* level0, const float* level1,
                         const float* level2, const float* level3, float* out, gsr_stream_t stream);
size_t gsr_flow_instance_norm_workspace_bytes(int N, int HW, int C);
int gsr_flow_instance_norm(int N, int HW, int C, const float* x, int relu, const float* residual, float* out, void* workspace,
                           gsr_stream_t stream);
int gsr_flow_gru_combine(long long P, int mode, const gsr_flow_slice* gate, const gsr_flow_slice* h, const gsr_flow_slice* q,
                         const gsr_flow_slice* out, gsr_stream_t stream);
int gsr_flow_upsample(int h8, int w8, const gsr_flow_slice* flow, const float* mask, int pad_top, int pad_left, int h, int w, float* out,
                      gsr_stream_t stream);

/* Tuning aid: when device_buffer is non-NULL (4*T uint64), the two blend kernels record the start/end wall
 * clock (100 MHz) of every workgroup: forward at [2*b], backward at [2*(T+b)], b = launch index.  NULL = off. */
int gsr_debug_set_trace(void* device_buffer);
/* Experiments: a launch order for the backward blend's units ([num_segments] unit ids by dispatch position; NULL: none). */
int gsr_debug_set_bwd_order(const void* device_order);
/* Tuning: workgroups per CU the runtime grants the exact / the planned preprocess kernel. */
int gsr_debug_preprocess_occupancy(int* exact, int* planned);

/* Per-kernel timing for benchmarks (no reference counterpart; the reference has no profiling hooks,
 * SURVEY.md section 5).  While enabled, every stage this thread launches is bracketed by HIP events
 * recorded on the launch stream.  gsr_profile_read waits for the recorded events and returns, per
 * stage (0 .. gsr_num_stages()-1, names from gsr_stage_name), the summed milliseconds and the number
 * of launches since the last reset.  ms, counts: [host] arrays of gsr_num_stages() entries. */
int gsr_num_stages(void);
const char* gsr_stage_name(int stage);
int gsr_profile_enable(int on);
int gsr_profile_read(float* ms, int* counts, int reset);

/* Host-side slack (benchmarks): nanoseconds this PROCESS has spent, summed over all threads, waiting for the stage-1
 * totals to arrive (the forward's one host synchronisation, rasterizer_impl.cu:281) since the last reset, and the number
 * of waits.  A step whose wait is near zero is bound by the host (Python, launches), not by the GPU.
 * wait_ns, waits: [host] out, may be NULL. */
int gsr_debug_host_wait(long long* wait_ns, long long* waits, int reset);

/* ---- Optimiser step.  gsr_adam_step replaces one parameter tensor's share of torch.optim.Adam.step() as GauSTAR
 * configures it (gaustar_scene/sugar_optimizer.py:87, :99-101; torch/optim/adam.py::_single_tensor_adam without weight
 * decay / amsgrad / maximize): in place on param, exp_avg, exp_avg_sq [n] f32 (16-byte aligned), grad [n] read only;
 * step = the 1-based count of this update (bias corrections 1 - beta^step).  Hyper-parameters are doubles, as the
 * reference holds them in Python floats: 1 - beta2 formed from a float32 beta2 would already be off by 1e-5. */
int gsr_adam_step(long long n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr, double beta1,
                  double beta2, double eps, int step, gsr_stream_t stream);
/* The same update for `count` tensors in one launch per 16 tensors (the optimiser of sugar_optimizer.py:67-87 holds eight
 * tensors, five of them a few MB: a launch each is mostly overhead).  numel, params, grads, exp_avgs, exp_avg_sqs, lrs:
 * [host] arrays of `count` entries (device pointers / element counts / per-tensor learning rates -- the groups differ in
 * nothing else); tensors with numel <= 0 are skipped.  Element for element the result of gsr_adam_step. */
int gsr_adam_step_multi(int count, const long long* numel, float* const* params, const float* const* grads,
                        float* const* exp_avgs, float* const* exp_avg_sqs, const double* lrs, double beta1, double beta2,
                        double eps, int step, gsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H_INCLUDED */
