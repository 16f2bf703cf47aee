/*
 * s2m2_hip.h -- C ABI of libs2m2_hip.so: hand-written CDNA4 (gfx950) kernels for the S2M2 inference hot path.
 *
 * The reference (junhong-3dv/s2m2) has no native/FFI layer: its hot path is the body of
 * S2M2.forward (src/s2m2/core/model/s2m2.py:136-197) expressed as ATen calls.  Every entry point below
 * replaces one group of those call sites (cited per function, SURVEY.md section 8a ids in brackets) and is what a
 * maintainer would bind from Python with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch); nothing is allocated inside;
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); all work is enqueued on it,
 *     no synchronisation, safe to capture in a hipGraph;
 *   - dtype codes: S2M2_F32 = 0, S2M2_F16 = 1;
 *   - return 0 on success, non-zero on error; s2m2_last_error() returns a thread-local message;
 *   - image-like activations are channels-last: (N, H, W, C) with C fastest ("NHWC"), tokens are rows;
 *   - thread-safe for distinct streams.
 */
#ifndef S2M2_HIP_H
#define S2M2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { S2M2_F32 = 0, S2M2_F16 = 1 };

/* ABI version of THIS header (major*10000 + minor*100 + patch).  s2m2_version() returns the value the library was built with: a caller
 * compares the two before its first call (s2m2_amd/hip.py: load() refuses a library whose value differs from the binding's: descriptor
 * layouts change IN PLACE between patch versions too, and a stale git-ignored .so would read pointers at shifted offsets).  The value is
 * bumped with EVERY change of a signature or descriptor layout.
 * History: 100 = rounds 1-2; 300 = round 3 changed signatures IN PLACE (cv_pitch inserted into s2m2_sinkhorn_regress / s2m2_cv_lookup,
 * s2m2_conv_desc / s2m2_chain_desc grew epi_cout0, ln_out*, fan_*, weight_frag, pool_h / pool_w) -- a caller built against 100 must be
 * rebuilt; 400 = round 4 (s2m2_pw_direct, s2m2_conv_narrow, s2m2_ln_corr_pitched added; the round-3 experiment entry
 * points s2m2_corr_tiled / s2m2_corr_hybrid / s2m2_debug_store_pattern and the ln_out_tile* fields of s2m2_chain_desc removed;
 * head_* appended to s2m2_narrow_desc without a bump -- the reason for the exact comparison since 500); 500 = round 5; 600 = round 6
 * (s2m2_row_attn and s2m2_conv_block added; the five ABI-400 entry points of K1 -- s2m2_ln_corr, _timed, _banded, _pitched, s2m2_corr -- removed: every form of
 * K1 is s2m2_cost_volume); 700 (engine files: s2m2_plan_save, s2m2_engine_*, s2m2_engine_region, s2m2_engine_info added; nothing changed
 * in place); 800 (s2m2_cloud, s2m2_cloud_workspace_bytes and s2m2_cloud_desc added: the 3D output stage behind the forward; nothing changed in place,
 * but engine files record the value and must be exported again); still 800 with s2m2_rectify and s2m2_rectify_desc (K16, the rectifier in front of
 * the forward): purely additive -- no existing struct or entry point changes, engine files do not contain the stage -- so neither callers nor
 * engine files of 800 are invalidated.  A library built before K16 reports 800 as well and lacks the symbol: s2m2_amd/hip.py load() names the
 * missing symbol and asks for a rebuild.  Still 800 with s2m2_disp_eval, s2m2_eval_workspace_bytes, s2m2_eval_tile_rows and s2m2_eval_desc (K18, the
 * evaluation stage behind the forward), added the same way, and with s2m2_mesh, s2m2_mesh_workspace_bytes, s2m2_mesh_tile_rows and s2m2_mesh_desc
 * (K20, the surface mesh behind the 3D stage), and with s2m2_register, s2m2_register_workspace_bytes and s2m2_register_desc (K21, the depth
 * map registered to a second camera), and with s2m2_segment, s2m2_segment_workspace_bytes, s2m2_segment_tile_rows, s2m2_segment_tile_cols and
 * s2m2_segment_desc (K22, connected components and the speckle filter), and with s2m2_voxel, s2m2_voxel_workspace_bytes, s2m2_voxel_tile_rows,
 * s2m2_voxel_home_slot and s2m2_voxel_desc (K23, voxel-grid downsampling of the point cloud). */
#define S2M2_ABI_VERSION 800
int s2m2_version(void);
const char* s2m2_last_error(void);
/* test aid (not part of the path): fills the LDS of every CU with quiet-NaN patterns, so that a kernel launched next that reads an LDS word it
 * never wrote produces NaNs instead of silently using stale data (tests/test_hip_lds_poison.py) */
int s2m2_debug_poison_lds(void* stream);
/* measurement aid (not part of the path): writes {shader-clock ticks (s_memtime), 100 MHz real-time ticks (s_memrealtime)} as two
 * uint64 to device memory `out`; two probes around a region of a stream give the average engine clock it ran at (tools/clock_probe.py) */
int s2m2_debug_clock_probe(void* out, void* stream);

/* Name of the device kernel s2m2_cost_volume dispatches to for this configuration (for rocprof matching). */
const char* s2m2_ln_corr_kernel_name(int C, int feat_dtype, int cv_dtype);

/*
 * [A4] K1: (LayerNorm +) all-pairs epipolar correlation = the cost volume  (DispInit.forward, submodules.py:216-217; LayerNorm :165)
 *   ONE descriptor for every form of the kernel (ABI 500; the five positional entry points of ABI 400 were removed with ABI 600):
 *   tokens  (2B, h, w, C) NHWC, left images = batch entries [0,B), right = [B,2B)            dtype token_dtype
 *   ln_weight, ln_bias  (C) fp32: LayerNorm affine (eps 1e-5, biased variance), applied INSIDE the kernel.  Both NULL: the tokens are
 *           normalised already (DispInit's layer_norm folded into the launch that produced them: the ln_out rows of s2m2_mlp_chain) and
 *           the kernel is the batched product R . L^T and its stores alone -- the shipped path at C = 128 / 192 / 256 / 384 in fp16
 *   cv      cv[b,y,i,j] = < LN(tokens[b,y,i,:]), LN(tokens[B+b,y,j,:]) >  at  cv + ((b*h + y)*w + i)*cv_pitch + j       dtype cv_dtype
 *   cv_pitch  elements between volume rows, >= w, a multiple of 8 (0 = w).  A multiple of 64 fp16 / 32 fp32 elements (w = 304 -> 320) makes
 *           every 64-column store granule a whole 128-byte line (then the stores are write-through, sc1); s2m2_sinkhorn_regress and
 *           s2m2_cv_lookup read the same pitch
 *   band    -1: the full volume.  >= 0 (use_positivity models): only columns j <= i + band are written (rounded up to the
 *           64-column store granule), the rest of the buffer is left untouched -- nothing downstream reads beyond band = 11: the Sinkhorn
 *           mask removes j > i (submodules.py:211-214), the +-4 tap lookups at both pyramid levels reach column i + 11 (submodules.py:39-60).
 *           The lookup of pixel i can also read ROW i - 1 at that column (the fp32 coordinate round trip lands just below i, weight ~1e-6):
 *           per row r the read set is j <= r + 12.  Row r + 12 > (r | 31) + 11 only where r % 32 == 31, and there the 64-column granule
 *           holds both columns (tests/test_hip_k3_edges.py pins it)
 *   start_event, stop_event  optional hipEvent_t (s2m2_event_create): recorded on the kernel dispatch itself (hipExtLaunchKernel), i.e. they
 *           bracket the kernel's execution like a rocprofv3 kernel trace does, not the gaps around it (bench.py `roofline`); elapsed time
 *           is valid once the stream has been synchronised
 *   C in {64,128,192,256,384}; w % 8 == 0.  F16: LN in fp32, operands rounded to fp16, fp32 accumulate (MFMA); F32: exact fp32 MFMA
 *   (v_mfma_f32_32x32x2_f32).  Pairs (token_dtype, cv_dtype): (F16,F16), (F16,F32), (F32,F32).
 */
typedef struct s2m2_corr_desc {
    const void* tokens;
    const float* ln_weight;
    const float* ln_bias;
    void* cv;
    int B, h, w, C;
    int cv_pitch;
    int band;
    int token_dtype, cv_dtype;
    void* start_event;
    void* stop_event;
} s2m2_corr_desc;
int s2m2_cost_volume(const s2m2_corr_desc* desc, void* stream);

/*
 * Weight packing into the MFMA-fragment orders of the direct-form kernels (ABI 500; up to ABI 400 these permutations lived in the Python
 * binding, s2m2_amd/pack.py, and a C caller had to re-derive them).  Input: the PLAIN packing of a layer -- (rows = Cout padded to 8, cols = K)
 * row-major fp16 with K = (tap, channel), channel fastest, every source's channel count padded to 8 (what
 * conv.weight.permute(0, 2, 3, 1).reshape(Cout, -1) gives for an unpadded layer; ld = elements between rows, 0 = cols).  Output: the stream the
 * kernel consumes, s2m2_pack_frag_elems() fp16 elements (-1: bad descriptor):
 *   S2M2_PACK_ROWS       s2m2_chain_desc.weight / fan_weight with weight_frag = 1 (K9; stack the layers of fan_weight along rows),
 *                        s2m2_pw_desc.weight_frag (K11): [row tile of 32][k16 step][lane][8], zero padded to whole tiles / steps
 *   S2M2_PACK_NARROW     s2m2_narrow_desc.weight_frag (K12), ntap = KH * KW: as ROWS; layers on >= 128 input channels in chunks of 64
 *   S2M2_PACK_CONV_FRAG  s2m2_conv_desc.weight with korder = 2 (K5 v5), ntap = KH * KW: [cout tile][channel chunk][tap][k16 step], chunks of
 *                        s2m2_conv_frag_chunk(rows, cols / ntap) channels (128; 192 for the layers of 192-channel models)
 *   S2M2_PACK_FUSION     s2m2_feature_fusion_frag's stream (K10): w = the first layers [feature_gate.0 ; feature_fusion.0] (3C, 2C) given as
 *                        rows = C, cols = 2C, w2 = [feature_gate.2 | feature_fusion.2] (C, 3C) (ld2: its row stride, 0 = 3C)
 *   S2M2_PACK_HEAD       s2m2_narrow_desc.head_frag: the 1x1 layer (rows <= 32 couts, cols = the 3x3 layer's couts) fused behind a K12 layer
 * One-time synchronous set-up (allocates and frees a small index map, waits for the stream): not for use under stream capture.
 */
enum { S2M2_PACK_ROWS = 0, S2M2_PACK_NARROW = 1, S2M2_PACK_CONV_FRAG = 2, S2M2_PACK_FUSION = 3, S2M2_PACK_HEAD = 4 };
/* channels per chunk of the K-order-2 stream of a layer (one input patch in LDS per chunk): 128, or 192 where that divides both sides and 128 does
 * not divide Cout (Cout = Cin = 192, 192 <- 384: blocks of 192 couts, no padded couts, no half-empty chunk).  Packers and s2m2_conv2d use this rule. */
static inline int s2m2_conv_frag_chunk(int cout, int cin) { return (cout % 128 != 0 && cout % 192 == 0 && cin % 192 == 0) ? 192 : 128; }
typedef struct s2m2_pack_desc {
    int kind;
    const void* w;
    const void* w2;
    int rows, cols;
    int ld, ld2;
    int ntap;
    void* out;
    long long out_elems;
} s2m2_pack_desc;
long long s2m2_pack_frag_elems(const s2m2_pack_desc* desc);
int s2m2_pack_frag(const s2m2_pack_desc* desc, void* stream);

/*
 * Recorded launch plans (ABI 500): a sequence of library calls replayed from C.  Between s2m2_plan_begin and s2m2_plan_end every launch-type entry
 * point the CALLING THREAD invokes is executed as always AND appended to the plan (arguments by value, descriptors copied).  s2m2_plan_end
 * declares the plan's EXTERNAL buffers -- next ranges [ext_base[i], ext_base[i] + ext_bytes[i]) of device memory: every recorded pointer into
 * range i is stored relative to it (ABI 600: only the pointer-typed arguments and the pointer fields of the descriptors are compared with the
 * ranges -- a size, a stride or a pair of ints that falls inside a range is never rewritten) -- and s2m2_plan_run re-issues the whole sequence
 * on `stream` with the externals at ext_ptrs[i] (same count
 * and order; a NULL external is accepted if no recorded call points into it).  All other pointers (weights, scratch, the intermediate tensors
 * of the recorded run) are replayed as recorded: the owner of the plan keeps those allocations alive and unshared for the life of the plan.
 * A plan is immutable once sealed; concurrent runs on different streams are safe when their externals differ and the caller accepts that the
 * internal intermediates are shared (i.e. in practice: one run at a time per plan).  Recording does not synchronise and may itself run under
 * stream capture; s2m2_plan_run may too.  s2m2_plan_abort ends a recording whose owner failed half way (the plan can only be destroyed then).
 *
 * s2m2_refine_step: ONE refinement iteration -- LocalRefiner.forward + the loop epilogue of S2M2.forward (refinenet.py:126-154, s2m2.py:175-180):
 * cost-volume lookup, the correlation / disparity / confidence feature layers, the refinement U-Net with its attention blocks, the ConvGRU, the
 * update heads, refine_update; about 55 launches -- as one native call: a plan recorded around that iteration whose seven externals are, in this
 * order, hidden (B,h,w,C), ctx (B,h,w,C), disp, conf, occ (B,1,h,w fp32), cv (B,h,w,cv_pitch) and the (B,h,w,8) side input written by the previous
 * iteration's epilogue (NULL for the first iteration, which builds its own).  The iteration's outputs are the tensors of the recorded run
 * (s2m2_amd/engine.py keeps them; a C caller records its own plan around its own launch sequence the same way).
 */
typedef struct s2m2_plan s2m2_plan;
int s2m2_plan_begin(s2m2_plan** plan);
int s2m2_plan_end(s2m2_plan* plan, const void* const* ext_base, const size_t* ext_bytes, int next);
int s2m2_plan_abort(s2m2_plan* plan);
int s2m2_plan_launches(const s2m2_plan* plan);
int s2m2_plan_patches(const s2m2_plan* plan, int slot);   /* recorded pointers that follow external `slot` (< 0: all): diagnostics */
int s2m2_plan_run(const s2m2_plan* plan, const void* const* ext_ptrs, int next, void* stream);
int s2m2_plan_destroy(s2m2_plan* plan);
int s2m2_refine_step(const s2m2_plan* step, const void* hidden, const void* ctx, const void* disp, const void* conf, const void* occ,
                     const void* cv, const void* side_input, void* stream);

/*
 * Engine files (ABI 700): one whole forward as a self-contained file, loaded and run with nothing but this library and the HIP runtime.
 *
 * s2m2_plan_save writes a sealed plan (recorded with next = 0) together with the device memory its calls point to.  The caller describes that
 * memory as `nregions` disjoint ranges [base, base + bytes):
 *   S2M2_REGION_CONTENT   the bytes are stored (read from the device here: the caller synchronises first); an all-zero range is stored as its
 *                         size only, a range no recorded call points into as its size only and is never allocated by the loader
 *   S2M2_REGION_SCRATCH   only the size is stored; the loader allocates it zero-filled
 *   S2M2_REGION_EXTERNAL  an input slot: the first external is the left image, the second the right one, (B,3,H,W) of meta->image_dtype.
 *                         Only the first call (s2m2_image_prep) may point into an external
 * Every pointer word of every call (the pointer mask of the plan) is stored as (region, offset) or as null; a non-null pointer word that falls
 * in no region fails the save with the call, its entry point and the word.  The impl pointer of a call is stored as its entry point's name and
 * mapped back by the loader through the library's table of recordable entry points (name, blob size).  meta->out_region / out_offset name the
 * (3, B, 1, out_h, out_w) fp32 result (disp, occ, conf).
 *
 * s2m2_engine_load validates the whole file on the host before any device call (magic, format version, S2M2_ABI_VERSION equal to the
 * library's, entry names and blob sizes, every pointer inside its region, region sizes against the file length), then checks that the
 * current device is a gfx950, allocates the regions (every region 4096-byte aligned) on it, uploads the content and zeroes the scratch.
 * s2m2_engine_run: left / right (B,3,H,W) in meta.image_dtype, disp / occ / conf (B,1,out_h,out_w) fp32, all device buffers of the caller
 * on the engine's device.  The first call (image prep) is issued eagerly from the caller's images; the rest runs eagerly on the first run,
 * is captured as a hipGraph on the second and replayed from then on (S2M2_GRAPH=0: every run eager); the maps are copied out with three
 * device-to-device copies on `stream`.  ONE RUN AT A TIME PER ENGINE (the intermediates belong to the engine; a concurrent run fails);
 * any number of engines may coexist, one per device and configuration or several on one device.
 */
enum { S2M2_REGION_CONTENT = 0, S2M2_REGION_SCRATCH = 1, S2M2_REGION_EXTERNAL = 2 };
typedef struct s2m2_engine_region {
    const void* base;
    unsigned long long bytes;
    int kind;
} s2m2_engine_region;
typedef struct s2m2_engine_info {
    int B, H, W;
    int dtype;                 /* compute dtype: S2M2_F32 / S2M2_F16 */
    int image_dtype;           /* S2M2_F32 / S2M2_F16 / 2 (uint8) */
    int feature_channels, dim_expansion, num_transformer;
    int use_positivity, output_upsample, refine_iter;
    int out_h, out_w;          /* (H, W), or (2H, 2W) with output_upsample */
    int out_region;
    long long out_offset;
} s2m2_engine_info;
typedef struct s2m2_engine s2m2_engine;
int s2m2_plan_save(const s2m2_plan* plan, const s2m2_engine_region* regions, int nregions, const s2m2_engine_info* meta, const char* path);
int s2m2_engine_load(const char* path, s2m2_engine** engine);
int s2m2_engine_meta(const s2m2_engine* engine, s2m2_engine_info* meta);
int s2m2_engine_run(s2m2_engine* engine, const void* left, const void* right, float* disp, float* occ, float* conf, void* stream);
int s2m2_engine_destroy(s2m2_engine* engine);

int s2m2_event_create(void** event);
int s2m2_event_destroy(void* event);
int s2m2_event_elapsed_us(void* start_event, void* stop_event, float* microseconds);

/*
 * [A5+A6] Sinkhorn optimal transport with dustbins + argmax + 5-tap window regression
 *   (DispInit._optimal_transport/_sinkhorn submodules.py:169-201, regression :225-241, logsumexp_stable :147-152)
 *   cv      (B, h, w, w) dtype cv_dtype (read only), volume rows cv_pitch elements apart (0 = w; a multiple of 8)
 *   disp, conf, occ  (B, h, w) fp32 out  (disp = i - soft-argmax, 1/4-res pixels; occ = row mass of masked P)
 *   argmax  (B, h, w) int32 out or NULL  (first maximal j wins)
 *   use_positivity: entries j > i are masked (the reference fills -1e4, which underflows to exactly 0 in fp32)
 *   workspace: NULL or >= s2m2_sinkhorn_workspace_bytes(...) bytes.
 */
size_t s2m2_sinkhorn_workspace_bytes(int B, int h, int w, int cv_dtype);
int s2m2_sinkhorn_regress(const void* cv, float* disp, float* conf, float* occ, int32_t* argmax,
                          int B, int h, int w, int ot_iter, int use_positivity, int cv_dtype, int cv_pitch,
                          void* workspace, void* stream);

/*
 * [A9+A10] two-level cost-volume lookup, radius r (CostVolume.__init__/__call__, submodules.py:23-60,
 *   bilinear_sampler :7-17).  Level 1 (cv averaged over pairs of j) is computed on the fly, never stored.
 *   cv    (B, h, w, w) dtype cv_dtype, volume rows cv_pitch elements apart (0 = w);  disp (B, h, w) fp32
 *   corr1, corr2  fp32 (or fp16 when out_dtype = S2M2_F16) with element (b,y,i,k) at
 *       base + ((b*h + y)*w + i)*pix_stride + k*tap_stride      k = 0..2r  <->  dx = k - r
 *   (planar (B,2r+1,h,w) of the reference: pix_stride=1, tap_stride=h*w with base offset b*(2r+1)*h*w handled by
 *    batch_stride; channels-last: pix_stride=2r+1 (or larger), tap_stride=1)
 *   The reference's pixel -> normalised -> pixel fp32 coordinate round trip (grid_sample, align_corners=True,
 *   zeros padding) is reproduced on both axes.
 *   w even and >= 4 (level 1 needs two columns); 0 <= r <= 16; B*h <= 65535 image rows per launch.
 */
int s2m2_cv_lookup(const void* cv, const float* disp, void* corr1, void* corr2,
                   int B, int h, int w, int radius, int cv_dtype, int out_dtype,
                   long long batch_stride, long long pix_stride, long long tap_stride, int cv_pitch, void* stream);

/*
 * [A2,A3,A7,A8,A11,A12,A14,A15] implicit-GEMM convolution / linear layer with fused concatenation and epilogues.
 *   Replaces the stride-1 nn.Conv2d / nn.ConvTranspose2d / nn.Linear call sites outside the CNN backbone
 *   (refinenet.py:14-20,47-57,87-122; attentions.py:24-28,71-74,239-241,269-275; feature_fusion.py:15-21;
 *   stacked_MRT.py:22-34; unet.py:25-37; submodules.py:104-108,127-135; s2m2.py:65-67) and the elementwise kernels
 *   PyTorch launches around them: torch.cat of the inputs, bias, GELU/ReLU/sigmoid/tanh, residual add, the ConvGRU gate
 *   arithmetic (refinenet.py:24-34), the FeatureFusion gate mix (feature_fusion.py:24-31).
 *
 *   out[n,y,x,co] = epi( out_scale * act( bias[co] + sum_{ky,kx,ci} in[n, y*stride+ky-KH/2, x*stride+kx-KW/2, ci] * weight[co,ky,kx,ci] ) )
 *   in  = channel concatenation of src[0..nsrc) (NHWC, src_c[s] channels each, pixel stride src_stride[s]; zero padding)
 *   weight  packed (Cout, KH*KW, Cin), Cin = sum(src_c), same dtype as the activations; bias fp32 (Cout) or NULL
 *   out NHWC with pixel stride out_stride (write into a channel slice of a wider tensor by offsetting `out`)
 *   every channel count / stride is a multiple of 8 (callers zero-pad: weights of padded channels are zero)
 *   epi: ADD  v + aux0 | MUL  v * aux0 | GRU  (1-aux0)*aux1 + aux0*v  (aux0 = z, aux1 = h, v = q)
 *        GATEMIX  g = clamp(v, .01, .99); g*aux0 + (1-g)*aux1          (aux tensors NHWC at the output pixel/channel)
 *        DUALMIX  two 1x1 layers on the same rows in one launch (the two heads of FeatureFusion, feature_fusion.py:15-31):
 *                 weight rows = [W1 (Cout x ksplit) | W2 (Cout x (Cin - ksplit))] along K, act = SIGMOID;
 *                 g = clamp(sigmoid(W1.in[:ksplit] + bias), .01, .99);  out = (W2.in[ksplit:] + bias2) + g*aux0 + (1-g)*aux1
 *   shuffle2 = C' > 0: the conv is the GEMM of a ConvTranspose2d(kernel 2, stride 2): KH = KW = 1, Cout = 4*C' ordered
 *        (dy, dx, c'), result stored to (N, 2H, 2W, C') with pixel stride out_stride.
 *   tile: 0 = automatic, 1..4 force a block tile (128x128, 64x64, 128x32, 128x64) -- tests and tuning only.
 */
enum { S2M2_ACT_NONE = 0, S2M2_ACT_GELU = 1, S2M2_ACT_RELU = 2, S2M2_ACT_SIGMOID = 3, S2M2_ACT_TANH = 4 };
enum { S2M2_EPI_NONE = 0, S2M2_EPI_ADD = 1, S2M2_EPI_MUL = 2, S2M2_EPI_GRU = 3, S2M2_EPI_GATEMIX = 4, S2M2_EPI_DUALMIX = 5 };
typedef struct s2m2_conv_desc {
    const void* src[4];
    int src_c[4];
    int src_stride[4];
    int nsrc;
    const void* weight;
    const float* bias;
    void* out;
    int out_stride;
    int N, H, W, KH, KW, Cout;
    int act, epi;
    const void* aux0;
    const void* aux1;
    int aux0_stride, aux1_stride;
    float out_scale;
    int shuffle2;
    int tile;
    int dtype;
    int korder;             /* K order of the packed weight: 0 = (Cout, KH, KW, Cin); 1 = (Cout, KH, Cin/CH, KW, CH) with CH = 64 bytes of
                               channels (32 fp16 / 16 fp32; Cin % CH == 0): horizontal taps become consecutive K tiles -> L1 reuse;
                               2 = fp16 MFMA fragment stream [Cout/32][ceil(Cin/CK)][KH*KW][CK/16][64 lanes][8] (lane l: cout 32t + l%32,
                               channel CK c + 16s + 8(l/32) + e; zero beyond Cin; CK = s2m2_conv_frag_chunk(Cout, Cin)) for stride-1
                               3x3 / 3x1 / 1x3 layers with Cout % 128 == 0, or Cout % 192 == 0 and Cin % 192 == 0:
                               the weights go from L2 straight into MFMA operands, only the input patch is staged in LDS */
    int stride;             /* 1 or 2: out[y,x] is centred on in[y*stride, x*stride]; output (N, ceil(H/stride), ceil(W/stride), Cout) */
    const float* ln_wsum;   /* non-NULL: the layer is LayerNorm(Cin, elementwise_affine=False, eps=ln_eps) followed by this 1x1 layer
                               (the pre-norm of attentions.py:117,148,182,213,243 feeding its Linear): `in` holds the RAW rows, the kernel
                               computes W.((x-mean)*rstd)+b as rstd*(W.x - mean*ln_wsum)+b with the row statistics taken inside the GEMM;
                               ln_wsum[co] = sum_k weight[co,k] (fp32, Cout entries, summed from the packed weight).
                               Needs KH = KW = 1, stride 1, no shuffle2, Cin with no padding channels, act NONE or GELU. */
    float ln_eps;
    int ksplit;             /* S2M2_EPI_DUALMIX: first K index (channel of `in`) of the second layer; multiple of 64 */
    const float* bias2;     /* S2M2_EPI_DUALMIX: bias of the second layer (fp32, Cout) or NULL */
    int pool2;              /* 1: the layer is nn.AvgPool2d(2) followed by this 1x1 layer (down_conv of Unet / MRT, reference unet.py:24-29,
                               stacked_MRT.py:21-26): a GEMM row is the mean of input pixels (2y, 2x) .. (2y+1, 2x+1), formed and rounded
                               to the I/O dtype exactly as s2m2_resample2x mode 0 does; output (N, H/2, W/2, Cout).  Needs KH = KW = 1,
                               stride 1, korder 0, no shuffle2 / ln_wsum / DUALMIX. */
    int epi_cout0;          /* > 0 (korder 2, one-operand epilogues ADD / MUL, a multiple of 128): the epilogue applies to couts >= epi_cout0
                               only, couts below it are stored after bias + activation -- two layers that read the same input stacked along
                               Cout with different epilogues in ONE launch (ConvGRU: z = sigmoid(convz(hx)) | r*h = sigmoid(convr(hx)) * h,
                               refinenet.py:24-29).  aux0 then has Cout - epi_cout0 channels: aux0[pixel * aux0_stride + (cout - epi_cout0)]
                               (ABI 500: the tensor's own base pointer; up to ABI 400 the caller passed it shifted by -epi_cout0 elements). */
} s2m2_conv_desc;
int s2m2_conv2d(const s2m2_conv_desc* desc, void* stream);

/*
 * K9 -- a chain of up to three 1x1 layers (nn.Linear / 1x1 nn.Conv2d, all C -> C) on token rows in ONE launch; the row tile
 *   stays in LDS between the layers.  Replaces, per transformer block, the attention output projection + residual and the FFN
 *   (reference attentions.py:311-321 GlobalAttnBlock.forward, :347-355 BasicAttnBlock.forward:  z = z + proj(o);
 *   z = z + ffn(norm(z)) with ffn = Linear-GELU-Linear, attentions.py:239-241), and the 1x1 branch of ConvBlock2D
 *   (attentions.py:269-275: Conv1x1-ReLU-Conv1x1).
 *
 *   t_0 = x rows;   y_s = act_s( W_s . (ln_wsum[s] ? LayerNorm(t_s) : t_s) + b_s );   if (s == res_stage) y_s += res rows;
 *   if (carry && s == 2) y_2 += y_0;   t_{s+1} = y_s;   out = y_{nstage-1}
 *   weight[s] packed (C, C) like s2m2_conv2d's 1x1 weight, bias fp32 (C) or NULL, ln_wsum[s] fp32 (C) row sums of weight[s]
 *   (non-NULL: LayerNorm without affine, eps ln_eps, folded in as in s2m2_conv2d); act NONE / GELU / RELU.
 *   Every y_s is rounded to the I/O dtype before it is used again, exactly as separate launches would store it.
 *   C: 128 / 256 / 384 / 512 (fp16), 128 / 256 (fp32): ask s2m2_mlp_chain_supported; row strides in elements, multiples of 8.
 */
typedef struct s2m2_chain_desc {
    const void* x;
    const void* res;
    void* out;
    long long x_stride, res_stride, out_stride, rows;
    int C, nstage;
    const void* weight[3];
    const float* bias[3];
    const float* ln_wsum[3];
    int act[3];
    int res_stage;          /* -1: no residual rows */
    int carry;
    float ln_eps;
    int dtype;
    /* optional second output of the last stage: ln_out rows = LayerNorm(out rows) * ln_gamma + ln_beta over the C channels (fp32
       statistics of the rounded `out` rows, biased variance, eps ln_out_eps, result rounded to the I/O dtype).  Folds DispInit's
       layer_norm (submodules.py:165,216) into the launch that produces feature_tr_4x; consumed by s2m2_corr.  NULL: none.
       Needs C * sizeof(dtype) / 16 in {16, 32, 64} (fp16: C = 128 / 256 / 512; fp32: C = 128 / 256). */
    void* ln_out;
    long long ln_out_stride;
    const float* ln_gamma;
    const float* ln_beta;
    float ln_out_eps;
    /* fan-out stages, nfan = 0: none.  nfan further C -> C layers that ALL read the chain's `out` rows (while they are still in LDS) and
       write fan_out[:, f*C:(f+1)*C] = W_f . (fan_ln_wsum ? LayerNorm(out rows) : out rows) + b_f  -- the Q | K | V projection of the attention
       block that follows (reference attentions.py:24-28,71-74 behind the pre-norm of :117,148), fused into the launch that produces its
       input: fan_weight packed (nfan*C, C), fan_bias fp32 (nfan*C) or NULL, fan_ln_wsum fp32 (nfan*C) row sums (eps ln_eps) or NULL. */
    const void* fan_weight;
    const float* fan_bias;
    const float* fan_ln_wsum;
    void* fan_out;
    long long fan_out_stride;
    int nfan;
    /* placement hint, 0 = none: the rows are `rows / (8 * xcd_group_rows)` images of 8 groups of xcd_group_rows consecutive rows each;
       group g of every image is processed on XCD g (blocks are dealt to XCDs round robin by the hardware), so that a consumer which
       places its work the same way -- s2m2_corr: image row y on XCD y / (h / 8) -- reads these rows from the L2 that holds them. */
    long long xcd_group_rows;
    /* 1: weight[s] and fan_weight are in MFMA-FRAGMENT order instead of row-major -- the same C x C (nfan*C x C) fp16 values, with the
       16-byte piece (cout o, channels 8q .. 8q+7) at 16-byte slot ((o/32) * (C/16) + q/2) * 64 + (q%2) * 32 + o%32 (per fan-out layer for
       fan_weight) -- and the launch runs the DIRECT form: a wave's weight fragments go from global memory straight into its MFMA operand
       registers, one whole stage ahead, no weight tile in LDS and no block barrier inside a stage.  For SHORT row counts (the 1/32 .. 1/8
       pyramid levels: a block lives for the latency of its weight stream, not for its arithmetic).  fp16, C = 128 / 192 / 256 / 384 / 512: ask
       s2m2_mlp_chain_frag_supported.  Same arithmetic and rounding points as the row-major form.  With nstage = 0 and nfan = 1 .. 4 the
       fan-out layers alone run in this form (any row count; nstage = 0 exists in this form only: ask s2m2_mlp_fan_supported). */
    int weight_frag;
    /* > 0 (with weight_frag): x is an image tensor (N, pool_h, pool_w, C) with pixel stride x_stride, and row m = (n, yo, xo) of the
       (pool_h/2, pool_w/2) grid is the mean of its four pixels (2yo, 2xo) .. (2yo+1, 2xo+1): nn.AvgPool2d(2) in front of the 1x1 layer(s)
       (the down_conv of Unet / MRT, reference unet.py:24-29, stacked_MRT.py:21-26) folded into the tile load, rounded to fp16 like the
       stand-alone pooling launch; rows = N * (pool_h/2) * (pool_w/2).  With chain stages (nstage >= 1, ABI 600) or fan-out only; residual,
       carry, ln_out and xcd_group_rows are not combined with it. */
    int pool_h, pool_w;
} s2m2_chain_desc;
int s2m2_mlp_chain_supported(int C, int dtype);
int s2m2_mlp_chain_frag_supported(int C, int dtype);
/* nstage = 0 with nfan > 0 ("fan-out only": the nfan layers read the x rows themselves -- a Q | K | V projection, or a pooled down_conv, as
 * ONE pass over the rows): 1 where the library has that form (the direct form, weight_frag = 1: fp16, C = 128 / 256, nfan 1..4), else 0 */
int s2m2_mlp_fan_supported(int C, int nfan, int dtype);
int s2m2_mlp_chain(const s2m2_chain_desc* desc, void* stream);

/*
 * K13 -- one whole 1-D (epipolar) attention step on token rows in ONE launch (ABI 600): pre-LayerNorm -> Q | K | V projections -> softmax
 *   attention along the image row -> output projection + residual -> pre-LayerNorm -> FFN (Linear - GELU - Linear) + residual.  Replaces, per
 *   step, the launch triple s2m2_mlp_chain(fan-out Q|K|V) / s2m2_attention / s2m2_mlp_chain of the reference's
 *   CrossAttnBlock1D + FFN and SelfAttnBlock1D + FFN (attentions.py:131-161, :99-128, :229-250; BasicAttnBlock.forward :347-355):
 *     z' = z + proj( softmax( (LN(z) Wq^T)(LN(s) Wk^T)^T / sqrt(d) ) (LN(s) Wv^T + bv) ),   out = z' + W2 GELU(W0 LN(z') + b0) + b2
 *   with z = a token row (image n, line y) and s = the same line of image (n + nimg/2) % nimg (cross = 1: left <-> right, shared weights, both
 *   directions in the launch) or z itself (cross = 0).  One block per token row; Q, K, V, the attention output and the FFN hidden tensor never
 *   leave the CU (K / V of the source row in LDS, everything else in registers).  Rounding points = those of the separate launches.
 *     x, out      (nimg, h, w, 128) fp16, channels contiguous; x_stride / out_stride = elements between tokens (multiples of 4); out != x
 *     weights     the six layers q, k, v, proj, ffn.0, ffn.2 back to back, 128 x 128 fp16 each (row = output channel) in the "row_attn
 *                 packing", 16-byte aligned, 32 KB per layer:
 *                 (1) columns: per 16 input channels the four quads of 4 channels in the order (0, 2, 1, 3) -- column 16g + 8a + 4b + e of the
 *                 plain packing (s2m2_conv2d's 1x1 weight) holds input channel 16g + 8b + 4a + e (a, b in {0, 1}, e < 4; an involution): the
 *                 k-slots of a 16-byte MFMA fragment then follow the accumulator layout of the layer before it;
 *                 (2) unit-major: the 16-byte unit u (columns 8u .. 8u+7 of (1)) of row r at element (u * 128 + r) * 8 of the layer -- the
 *                 kernel copies a layer into LDS with a linear LDS-DMA and reads conflict-free fragments at immediate offsets
 *     vectors     twelve fp32 vectors of 128 back to back, 16-byte aligned (absent biases as zeros): 0 bias q, 1 row sums of q, 2 bias k,
 *                 3 row sums of k, 4 bias v, 5 row sums of v, 6 bias proj, 7 bias ffn.0, 8 row sums of ffn.0, 9 bias ffn.2, 10 ln_out gamma,
 *                 11 ln_out beta.  Row sums (of the plain fp16 weight, in fp32) fold the LayerNorm without affine (eps ln_eps) in front
 *                 of q, k, v, ffn.0 as in s2m2_conv2d (ln_wsum); 10 / 11 are used only with ln_out
 *     ln_out      optional second output: LayerNorm(out) * gamma + beta (eps ln_out_eps) -- DispInit's layer_norm (submodules.py:165,216)
 *                 when this step writes feature_tr_4x, as s2m2_chain_desc.ln_out
 *     xcd_hint    1 (h % 8 == 0): line y of every image runs on XCD y / (h / 8) -- where s2m2_cost_volume reads the rows (see
 *                 s2m2_chain_desc.xcd_group_rows) and where the partner row's block runs
 *   fp16, C = 128, heads 1 or 2 (head dim 128 / 64), 8 <= w <= 320: ask s2m2_row_attn_supported.
 */
typedef struct s2m2_rowattn_desc {
    const void* x;
    long long x_stride;
    void* out;
    long long out_stride;
    int nimg, h, w, C;
    int heads;
    int cross;
    const void* weights;
    const float* vectors;
    float ln_eps;
    void* ln_out;
    long long ln_out_stride;
    float ln_out_eps;
    int xcd_hint;
    int dtype;
} s2m2_rowattn_desc;
int s2m2_row_attn_supported(int C, int heads, int w, int dtype);
int s2m2_row_attn(const s2m2_rowattn_desc* desc, void* stream);

/*
 * K14 -- a whole ConvBlock2D (attentions.py:255-281) in ONE launch, for the coarse pyramid levels (ABI 600):
 *     out = convs.2( GELU( convs.0(x) ) ) + convs_1x.2( ReLU( convs_1x.0(x) ) )          convs.* 3x3 (padding 1), convs_1x.* 1x1, all C -> C
 *   Replaces the launch triple s2m2_mlp_chain (1x1 branch) / s2m2_conv2d (korder 2) / s2m2_conv2d (korder 2, EPI_ADD) with the same arithmetic
 *   in the same order (bit-identical): a block owns a patch of output pixels and all C channels, recomputes the one-pixel ring of the first
 *   3x3 layer and keeps the GELU tensor in LDS.  Meant for grids whose launches are latency chains (1/8 ... 1/32 resolution).
 *     x, out     (N, H, W, C) fp16, channels contiguous, x 16-byte and out 8-byte aligned, pixel strides in elements (at least C; x: multiple
 *                of 8, out: multiple of 4); out must not overlap x
 *     w_conv0/2  the 3x3 layers as s2m2_conv_desc.weight with korder = 2 (s2m2_pack_frag S2M2_PACK_CONV_FRAG, 128-channel chunks)
 *     w_1x0/2    the 1x1 layers as s2m2_chain_desc.weight with weight_frag = 1 (S2M2_PACK_ROWS)
 *     b_*        fp32 (C) or NULL
 *     patch_rows 0 = the library's choice; 2 / 4 force the patch height (C = 128; C = 256 runs 2-row patches)
 *   fp16, C = 128 / 256: ask s2m2_conv_block_supported.
 */
typedef struct s2m2_convblock_desc {
    const void* x;
    long long x_stride;
    void* out;
    long long out_stride;
    int N, H, W, C;
    const void* w_conv0;
    const void* w_conv2;
    const void* w_1x0;
    const void* w_1x2;
    const float* b_conv0;
    const float* b_conv2;
    const float* b_1x0;
    const float* b_1x2;
    int patch_rows;
    int dtype;
} s2m2_convblock_desc;
int s2m2_conv_block_supported(int C, int H, int W, int dtype);
int s2m2_conv_block(const s2m2_convblock_desc* desc, void* stream);

/*
 * K17 -- one ConvGRU half (refinenet.py:7-36) in ONE launch (ABI still 800: additive):
 *     z = sigmoid(convz([h, x]))   r = sigmoid(convr([h, x]))   q = tanh(convq([r * h, x]))   out = (1 - z) * h + z * q
 *   with KH x KW = 3 x 1 or 1 x 3 taps (zero padding), hidden and input width C.  Replaces the launch pair s2m2_conv2d (korder 2, the stacked
 *   z | r layer with epi_cout0 = C and the r * h epilogue) / s2m2_conv2d (the candidate layer with S2M2_EPI_GRU) with the same arithmetic in
 *   the same order (bit-identical to the pair with the candidate layer in K order 2): a block owns a patch of output pixels, recomputes r on
 *   the patch's one-pixel ring along the tap axis and keeps z and r * h on the CU.
 *     h, x, out  (N, H, W, C) fp16, channels contiguous, 16-byte aligned, pixel strides in elements (at least C, multiples of 8); out must
 *                not overlap h or x
 *     w_zr       [convz | convr] stacked along Cout (2 C rows, z first) over cat(h, x), as s2m2_conv_desc.weight with korder = 2
 *     w_q        convq over cat(r * h, x), as s2m2_conv_desc.weight with korder = 2
 *     b_zr, b_q  fp32 (2 C) / (C), or NULL
 *   fp16, C = 128: ask s2m2_conv_gru_supported.
 */
typedef struct s2m2_convgru_desc {
    const void* h;
    long long h_stride;
    const void* x;
    long long x_stride;
    void* out;
    long long out_stride;
    int N, H, W, C;
    int KH, KW;
    const void* w_zr;
    const void* w_q;
    const float* b_zr;
    const float* b_q;
    int dtype;
} s2m2_convgru_desc;
int s2m2_conv_gru_supported(int C, int H, int W, int dtype);
int s2m2_conv_gru(const s2m2_convgru_desc* desc, void* stream);

/*
 * K19 -- the second half of a ConvBlock2D (attentions.py:255-281) in ONE launch, for the grids K14 does not take (ABI still 800: additive):
 *     out = fp16( fp16(convs.2(t) + b_conv2) + fp16(convs_1x.2( fp16(ReLU(convs_1x.0(z) + b_1x0)) ) + b_1x2) )
 *   t = GELU(convs.0(z)) comes from the unchanged s2m2_conv2d launch.  Replaces the launch pair s2m2_mlp_chain (the two-stage 1x1 branch,
 *   weight_frag = 1) / s2m2_conv2d (korder 2, S2M2_EPI_ADD on the chain's output) with the same arithmetic in the same order (bit-identical):
 *   the 1x1 branch needs no halo, so the block that will add it computes it on its own patch in front of the 3x3 layer's K loop.
 *     t, z, out   (N, H, W, C) fp16, channels contiguous, 16-byte aligned, pixel strides in elements (at least C, multiples of 8); out must
 *                 not overlap t or z
 *     w_conv2     the 3x3 layer as s2m2_conv_desc.weight with korder = 2 (s2m2_pack_frag S2M2_PACK_CONV_FRAG, 128-channel chunks)
 *     w_1x0/2     the 1x1 layers as s2m2_chain_desc.weight with weight_frag = 1 (S2M2_PACK_ROWS)
 *     b_*         fp32 (C) or NULL
 *     patch_rows x patch_cols   0 x 0 = the library's choice (csrc/convtail_select.h); 2 x 32, 4 x 32, 4 x 40 force the block's pixel patch
 *   fp16, C = 128 / 256: ask s2m2_conv_block_tail_supported.
 */
typedef struct s2m2_convtail_desc {
    const void* t;
    long long t_stride;
    const void* z;
    long long z_stride;
    void* out;
    long long out_stride;
    int N, H, W, C;
    const void* w_conv2;
    const void* w_1x0;
    const void* w_1x2;
    const float* b_conv2;
    const float* b_1x0;
    const float* b_1x2;
    int patch_rows, patch_cols;
    int dtype;
} s2m2_convtail_desc;
int s2m2_conv_block_tail_supported(int C, int H, int W, int dtype);
int s2m2_conv_block_tail(const s2m2_convtail_desc* desc, void* stream);

/*
 * K11 -- a 1x1 layer with any channel counts in the direct style (fp16; round 4): Conv2d(kernel 1) / Linear / ConvTranspose2d(2, stride 2) on
 *   up to four channel-concatenated sources (reference: LocalRefiner's corr_feat / conf_occ_feat / disp_corr_ctx_cat 1x1 layers,
 *   refinenet.py:87-106,138-146; the up_conv 1x1 layers of Unet / MRT on the coarse grid, unet.py:32-37, stacked_MRT.py:29-34; the
 *   ConvTranspose heads of the upsampling masks, submodules.py:104-113,131-144), bias, NONE / GELU / RELU.
 *     out[m, :] = act(W . cat_i(src_i[m, :]) + bias)      rows m of `rows` tokens; src_i: src_c[i] channels (multiples of 8), row stride
 *   src_stride[i]; K = sum src_c, K rounded up to 16 in {32, 48, 64, 96, 128, 192, 256, 384}; Cout a multiple of 8 with 1, 2, 3, 4, 6 or 8
 *   32-cout tiles: ask s2m2_pw_direct_supported(K, Cout, dtype).
 *   weight_frag: the (Cout, K) weight zero-padded to (32 * tiles, 16 * steps) in MFMA-fragment order -- 16-byte slot (t * steps + s) * 64 + l
 *   holds row 32 t + l % 32, columns 16 s + 8 (l / 32) .. + 7 (pack.pw_frag); bias fp32 (Cout) or NULL.
 *   shuffle2 > 0: the ConvTranspose2d(2, s 2) store of s2m2_conv_desc (Cout = 4 * shuffle2, rows = N * Ho * Wo input pixels).
 */
typedef struct s2m2_pw_desc {
    const void* src[4];
    int src_c[4];
    long long src_stride[4];
    int nsrc;
    long long rows;
    const void* weight_frag;
    const float* bias;
    void* out;
    long long out_stride;
    int Cout;
    int act;
    int shuffle2, Ho, Wo;
    int dtype;
} s2m2_pw_desc;
int s2m2_pw_direct_supported(int K, int Cout, int dtype);
int s2m2_pw_direct(const s2m2_pw_desc* desc, void* stream);

/*
 * K12 -- spatial convolutions on NARROW inputs in the direct style (fp16; round 4): Conv2d / stride-1 ConvTranspose2d (as a convolution with
 *   the flipped kernel) whose input has exactly 8 or 16 channels -- one or two 16-byte pieces per pixel (reference: UpsampleMask1x
 *   conv_disp.0 | conv_rgb.0, submodules.py:124-129,139-141; LocalRefiner disp_feat.0 | conf_occ_feat.0, refinenet.py:93-101,141-142;
 *   CNNEncoder conv1_down.0, submodules.py:69-71).  Shapes: 3x3 stride 1 on 8 channels (any Cout % 8 == 0), 5x5 stride 2 on 16 channels
 *   (an even number of 32-cout tiles), and the second form below: ask s2m2_conv_narrow_supported (Cin = all input channels).  Padding K / 2, Ho = ceil(H / stride) as s2m2_conv2d.
 *     out[n, y, x, :] = act(sum_taps W[:, tap, :] . x[n, y*s - K/2 + ky, x*s - K/2 + kx, :] + bias)        act: NONE / GELU / RELU
 *   x: (N, H, W, Cin) with pixel stride x_stride (elements, multiple of 8); out: (N, Ho, Wo, Cout), pixel stride out_stride.
 *   weight_frag: the (Cout, KH*KW*Cin) matrix of s2m2_conv2d's K order 0 (K = (tap, channel)) zero-padded to (32 * tiles, 16 * steps) in
 *   MFMA-fragment order, as for K11 (pack.pw_frag); bias fp32 (Cout) or NULL.
 *   Second form, same entry point -- 3x3 stride 1 with FEW OUTPUT channels on wider inputs (UpsampleMask1x conv_concat.0, submodules.py:
 *   133-137,143; LocalRefiner disp_feat.2 and disp_update.2 | conf_occ_update.2, refinenet.py:93-96,108-118; GlobalRefiner out_feat,
 *   refinenet.py:61-66): Cin = 48 (Cout <= 64), 96 (Cout <= 96), 128 / 256 (Cout <= 32), from one or two channel-concatenated sources
 *   (x, x1).  Cin = 128 / 256: the K columns of the weight matrix chunk-major, K = (chunk of 64 channels, tap, channel) (pack.narrow_frag).
 */
typedef struct s2m2_narrow_desc {
    const void* x;
    long long x_stride;
    int N, H, W, Cin;                  /* Cin: ALL input channels (x holds the first Cin - Cin1 of them) */
    const void* x1;                    /* second source: channels [Cin - Cin1, Cin), pixel stride x1_stride; Cin1 = 0: none */
    long long x1_stride;
    int Cin1;
    const void* weight_frag;
    const float* bias;
    void* out;
    long long out_stride;
    int Cout, KH, KW, stride;
    int act;
    int dtype;
    /* fused 1x1 head (Cin = 48 form only; UpsampleMask1x conv_concat.0 -> ReLU -> conv_concat.2, submodules.py:133-137,143-144):
       head_cout > 0 (act NONE or RELU): out holds  W2 . act(conv3x3(x) + bias) + head_bias  with head_cout (multiple of 8, <= 32) channels instead of the Cout
       channels of the 3x3 layer, which are rounded to fp16 as a store would round them and never leave the registers.  head_frag: the
       (head_cout, Cout) matrix W2, rows zero-padded to 32, K columns zero-padded to 32-channel tiles and ordered to match the accumulator layout
       of the 3x3 layer: k16 step (j, p), j = channel / 32, p < 2; 16-byte slot ((j * 2 + p) * 64 + l) holds row l % 32 and the channels
       32 j + 8 (2 p + q) + 4 (l / 32) + e for q = 0, 1 and e = 0 .. 3, in that order (pack.head_frag). */
    const void* head_frag;
    const float* head_bias;
    int head_cout;
} s2m2_narrow_desc;
int s2m2_conv_narrow_supported(int KH, int KW, int stride, int Cin, int Cout, int dtype);
int s2m2_conv_narrow(const s2m2_narrow_desc* desc, void* stream);

/*
 * K10 -- FeatureFusion with 1x1 kernels in ONE launch (reference feature_fusion.py:4-33 with kernel_size = 1: every fusion of
 *   Unet / MRT, unet.py:39-41, stacked_MRT.py:36-41), the 3C-wide hidden tensor never leaves the CU:
 *     h = GELU(w1 . cat(z0, z1) + b1);  g = clamp(sigmoid(Wg . h[:C] + bg), .01, .99);  out = (Wf . h[C:] + bf) + g*z0 + (1-g)*z1
 *   z0, z1, out: `rows` token rows of C channels (row strides in elements, multiples of 8), dtype `dtype`;
 *   w1 packed (3C, 2C): rows [0,C) = feature_gate.0, rows [C,3C) = feature_fusion.0;  w2 packed (C, 3C) = [Wg (C,C) | Wf (C,2C)]
 *   along K;  b1 (3C), bg (C), bf (C) fp32.  C = 128 or 256: ask s2m2_feature_fusion_supported.
 *   z1_coarse_h / z1_coarse_w > 0: z1 is the COARSE tensor (N, z1_coarse_h, z1_coarse_w, C) and the kernel reads it through
 *   nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False) (unet.py:32-37: the up_conv feeding every decoder fusion);
 *   rows = N * 2*z1_coarse_h * 2*z1_coarse_w in raster order.  0 / 0: z1 has one row per output row.
 */
int s2m2_feature_fusion_supported(int C, int dtype);
int s2m2_feature_fusion(const void* z0, const void* z1, void* out, long long z0_stride, long long z1_stride, long long out_stride,
                        long long rows, int C, const void* w1, const float* b1, const void* w2, const float* bg, const float* bf,
                        int z1_coarse_h, int z1_coarse_w, int dtype, void* stream);
/*
 * K10, direct form (fp16, C = 128 / 256: ask s2m2_feature_fusion_frag_supported) for SHORT row counts: the same block, with the weights of
 *   both layers as ONE stream of 1 KB MFMA fragments per 32-cout tile, in the order the kernel consumes them, read from global memory
 *   straight into the operand registers (no weight tile in LDS, 6 block barriers per block instead of one per 64-byte K chunk).
 *   w_stream: 9*C*C fp16 values; fragment j of cout tile t at 16-byte slot (t * 9C/16 + j) * 64 + lane, lane l holding 8 consecutive K
 *   elements (k16 step, half l/32) of row 32t + l%32 of:  for slice s = 0, 1, 2:  w1 rows [sC, sC + C) (k16 steps 0 .. 2C/16),  then
 *   w2 = [Wg | Wf] columns [sC, sC + C) (steps 0 .. C/16)  -- w1, w2 as in s2m2_feature_fusion.  Same arithmetic and rounding points.
 */
int s2m2_feature_fusion_frag_supported(int C, int dtype);
int s2m2_feature_fusion_frag(const void* z0, const void* z1, void* out, long long z0_stride, long long z1_stride, long long out_stride,
                             long long rows, int C, const void* w_stream, const float* b1, const float* bg, const float* bf,
                             int z1_coarse_h, int z1_coarse_w, int dtype, void* stream);

/*
 * [A2,A3] pre-norm LayerNorm without affine over the channel axis (attentions.py:117,148,182,213,243; eps 1e-5, biased var).
 *   x, y: `rows` token rows of C channels, row strides x_stride / y_stride elements (multiples of 8); fp32 arithmetic.
 */
int s2m2_layernorm(const void* x, void* y, long long rows, int C, long long x_stride, long long y_stride, int dtype, void* stream);

/*
 * [A1] nn.GroupNorm(G, C) with affine on an NHWC activation (CNNEncoder, submodules.py:80,90).  x, y: (N, HW, C);
 *   gamma, beta fp32 (C); workspace >= s2m2_groupnorm_workspace_bytes(N, G) bytes (zeroed inside, on the stream).
 *   Statistics are accumulated in fp64, the normalisation runs in fp32.
 */
size_t s2m2_groupnorm_workspace_bytes(int N, int G);
int s2m2_groupnorm_nhwc(const void* x, void* y, const float* gamma, const float* beta, void* workspace, int N, long long HW,
                        int C, int G, float eps, int dtype, void* stream);

/*
 * [A14,A15 tails] convex upsampling (S2M2.upsample4x / upsample1x, s2m2.py:101-133; custom_unfold utils.py:9-20):
 *   out[m][b,Y,X] = scale[m] * sum_{n<9} softmax_n(logits[b,Y,X,0:9]) * x[m][b, clamp(Y/factor + n/3 - 1), clamp(X/factor + n%3 - 1)]
 *   x[m]   (B, hs, ws) fp32, m < nmaps <= 3 (host array of device pointers);  out[m] (B, hs*factor, ws*factor) fp32
 *   logits NHWC at the OUTPUT resolution, 9 used channels, rows padded to logit_stride >= 16 elements, dtype `dtype`;
 *   logit_up2 = 1 (output_upsample, s2m2.py:123-127): logits are (B, hs, ws, .) and bilinearly upsampled x2
 *   (align_corners=False, rounded to `dtype`) on the fly; factor must be 2.
 *   chan_out != NULL: map 0 is also stored, in `dtype`, at chan_out[pixel * chan_stride] (the disparity input channel of
 *   UpsampleMask1x, submodules.py:137, written straight into the 8-channel image tensor).
 */
int s2m2_convex_upsample(const float* const* x, float* const* out, const float* scale, int nmaps, const void* logits,
                         int logit_stride, int B, int hs, int ws, int factor, int logit_up2, void* chan_out,
                         long long chan_stride, int dtype, void* stream);

/*
 * [A2,A3] multi-head attention softmax(Q K^T * scale) V, flash style (no score matrix in memory).  Replaces
 *   F.scaled_dot_product_attention and the explicit attention + positional-encoding einsums (attentions.py:42-50, :83-91).
 *   q, k, v, out: token rows; element (batch b, token n, head hd, e) at base + (b*N + n)*stride + hd*D + e  (so the fused
 *   QKV projection is read in place and the output is (tokens, heads*D)).  D multiple of 8, <= 384 (<= 128 with PE).
 *   swap_halves = 1: keys/values of batch b come from batch (b + nb/2) % nb (symmetric cross attention, CrossAttn).
 *   pe_x != NULL selects SelfAttn(use_pe=True): tokens form a grid_h x grid_w grid (row major), pe_x (2*grid_w-1, 16) and
 *   pe_y (2*grid_h-1, 16) fp32 are the separable sinc tables of get_pe (utils.py:32-60) indexed by xq-xk+grid_w-1 /
 *   yq-yk+grid_h-1, and pe_out (tokens, heads*32) receives sum_k P[q,k] * 0.5*[pe_x[..], pe_y[..]]  (the input of pe_proj).
 */
int s2m2_attention(const void* q, const void* k, const void* v, void* out, long long q_stride, long long k_stride,
                   long long v_stride, long long out_stride, int nb, int heads, int Nq, int Nk, int D, float scale,
                   int swap_halves, const float* pe_x, const float* pe_y, void* pe_out, long long pe_stride,
                   int grid_w, int grid_h, int dtype, void* stream);
/*
 * Plans the launch s2m2_attention would make for (nb, heads, N = Nq = Nk, D, dtype) -- head-dim instantiation, and for the PE variant
 *   (grid_w, grid_h > 0; 0, 0 = no positional encoding) the marginal-bin tiles, waves per block and the 160 KB LDS budget -- without
 *   launching.  1 = supported, 0 = not (s2m2_last_error names the limit).  Lets the host reject a geometry BEFORE the first launch of a
 *   forward (token grids above 96 x 96 cells = images above 3072 px per side have no PE instantiation).
 */
int s2m2_attention_supported(int nb, int heads, int N, int D, int grid_w, int grid_h, int dtype);
/*
 * The launch s2m2_attention would make for this call, as its own planning code decides it (the walk of s2m2_attention_supported with Nq, Nk
 *   and swap_halves given): the kernel instantiation -- padded head dim, fewest waves a block is built for, key-split mode, PE bin tiles
 *   (0, 0 without PE), 32-key sub-tiles per stage, two-sweep softmax, queries in LDS, two stages in flight -- and the launch: waves per block,
 *   query blocks per (batch, head), dynamic LDS bytes.  Host code only.  0 = planned, otherwise s2m2_last_error says why not (`*plan` zeroed).
 *   tests/test_k4_cases_cpu.py holds every case of the K4 plan tests to what this entry reports.
 */
typedef struct s2m2_attn_plan {
    int dp, minw, ksplit, nxt, nyt, nw, nblk, kt, twopass, qlds, deep;
    long long lds_bytes;
} s2m2_attn_plan;
int s2m2_attention_plan(int nb, int heads, int Nq, int Nk, int D, int swap_halves, int grid_w, int grid_h, int dtype, s2m2_attn_plan* plan);

/*
 * [A2,A3] 2x resampling of an NHWC activation: mode 0 = nn.AvgPool2d(2) (unet.py:25-30, stacked_MRT.py:22-27), mode 1 =
 *   bilinear x2 with align_corners=False (unet.py:32-37, stacked_MRT.py:29-34).  x (N,H,W,C) -> y (N,H/2,W/2,C) or (N,2H,2W,C),
 *   pixel strides x_stride / y_stride elements; fp32 arithmetic.
 */
int s2m2_resample2x(const void* x, void* y, int N, int H, int W, int C, long long x_stride, long long y_stride, int mode,
                    int dtype, void* stream);

/*
 * [A0,A7,A11,A13] fused per-pixel stages between the big kernels (each is a chain of separate elementwise kernels in PyTorch):
 *   s2m2_image_prep     normalize_img (s2m2.py:80-89) + left/right concat (:143) + NHWC packing: img0, img1 (B,3,H,W) planar,
 *                       img_dtype S2M2_F32 / S2M2_F16 / 2 (uint8), values in [0,255] -> x8 (2B,H,W,8) with channels 1..3 =
 *                       (v/255 - 0.5)*2 and channels 0, 4..7 = 0 (channel 0 later carries the upsampled disparity, A15)
 *   s2m2_refine_prep    mode 0 (GlobalRefiner, refinenet.py:63-68): small8[...,0] = disp/100*mask, [...,1] = logit(mask*conf, 0.1),
 *                       mask = conf > 0.2;  mode 1 (LocalRefiner, :134-141): disp/100, logit(conf, 0.01), logit(occ, 0.01)
 *   s2m2_global_update  out = mask*disp + (1-mask)*upd*100 [clamped at 0]  (refinenet.py:70-71, s2m2.py:160-161); upd = channel 0
 *                       of an NHWC tensor with pixel stride upd_stride
 *   s2m2_refine_update  in place: disp += dco[0]; conf = sigmoid(dco[8] + logit(conf, .01)); occ likewise with dco[9]
 *                       (refinenet.py:149-151); then clamp disp at 0 if use_positivity and occ *= (x - disp >= 0) (s2m2.py:177-180)
 *   s2m2_refine_update_to  the same out of place (outputs may alias the inputs); small8_next != NULL also receives the mode-1
 *                       side input of the next refinement iteration (= s2m2_refine_prep of the values just written, bit for bit)
 *   s2m2_tanh           y = tanh(x) on n elements (hidden = tanh(ctx), s2m2.py:166)
 *   s2m2_stem_mlp       the two 1x1 layers at the head of CNNEncoder on full-resolution pixels (submodules.py:68-71: conv0 =
 *                       Conv2d(3,16,1) - GELU - Conv2d(16,16,1)): x8 (npix,8) -> out (npix,16) = W1.gelu(W0.x + b0) + b1;
 *                       w0 (16,8), w1 (16,16), biases (16): fp32, weights already rounded to the activation dtype
 *   disp, conf, occ, out: (B,h,w) fp32.
 */
int s2m2_image_prep(const void* img0, const void* img1, void* x8, int B, int H, int W, int img_dtype, int dtype, void* stream);
int s2m2_refine_prep(const float* disp, const float* conf, const float* occ, void* small8, long long npix, int mode, int dtype, void* stream);
int s2m2_global_update(const void* upd, int upd_stride, const float* disp, const float* conf, float* out, long long npix, int clamp0,
                       int dtype, void* stream);
int s2m2_refine_update(const void* dco, int dco_stride, float* disp, float* conf, float* occ, long long npix, int w, int use_positivity,
                       int dtype, void* stream);
int s2m2_refine_update_to(const void* dco, int dco_stride, const float* disp, const float* conf, const float* occ, float* disp_out,
                          float* conf_out, float* occ_out, void* small8_next, long long npix, int w, int use_positivity, int dtype,
                          void* stream);
int s2m2_tanh(const void* x, void* y, long long n, int dtype, void* stream);
int s2m2_stem_mlp(const void* x8, const float* w0, const float* b0, const float* w1, const float* b1, void* out, long long npix, int dtype,
                  void* stream);

/*
 * [8f-1] image_pad of the reference driver (src/s2m2/core/utils/image_utils.py:27-71), on the device: (B,C,H,W) planar image
 *   (img_dtype S2M2_F32 / S2M2_F16 / 2 = uint8) -> out (B,C,Hn,Wn) fp32, Hn/Wn = H/W rounded up to multiples of `factor`, the
 *   original image centred (offset (Hn-H)/2, (Wn-W)/2); the border = bilinear (align_corners=False) upsampling of the adaptive
 *   average pooling of the zero-padded image to (H/factor, W/factor).  pooled: scratch (B,C,H/factor,W/factor) fp32.
 */
int s2m2_image_pad(const void* img, float* pooled, float* out, int B, int C, int H, int W, int factor, int img_dtype, void* stream);

/*
 * K15 -- the 3D output stage behind the forward: validity filter, metric depth and a compacted coloured point cloud, on the device.
 *   Replaces the host-side numpy / open3d steps of the reference's demos (demo/visualize_3d_middlebury.py:32-52,97-107: get_pointcloud and
 *   the filtered disparity; src/s2m2/core/utils/model_utils.py:111-136; the validity mask of src/s2m2/core/utils/vis_utils.py:62; open3d's
 *   RGBDImage.create_from_color_and_depth + PointCloud.create_from_rgbd_image by their documented behaviour).
 *     disp, occ, conf  (B,1,Hp,Wp) fp32: the padded maps as S2M2.forward / s2m2_engine_run return them
 *     image            (B,3,H,W) planar left image, UNPADDED, image_dtype S2M2_F32 / S2M2_F16 / 2 (uint8), values in [0,255].  The crop of
 *                      image_crop is fused: image pixel (v,u) reads map pixel (v + (Hp-H)/2, u + (Wp-W)/2); H == Hp, W == Wp is fine
 *   per pixel, all in fp32 (u, v: pixel indices of the unpadded image):
 *     valid = unfiltered || (conf > conf_min && occ > occ_min);       d = valid ? disp : -1
 *     depth = d <= 0 ? 1e9f : (float)(baseline * fx) / (d + (float)doffs)             (the product baseline * fx is formed in double here)
 *     z = depth / depth_scale;      keep = z > 0 && z < depth_trunc                   (depth_trunc <= 0: 1e9, the reference's None)
 *     x = (u - cx) * z / fx;        y = (v - cy) * z / fy
 *     r, g, b = the pixel's colour as bytes (fp16 / fp32 images: clamped to [0,255], rounded to nearest even)
 *   outputs, each optional (NULL), at least one:
 *     depth    (B,1,H,W) fp32: z where keep, else 0
 *     mask     (B,1,H,W) uint8: keep
 *     count    (B) int32: the number of kept pixels of every pair -- ALWAYS the true number, also above `capacity`.  Non-NULL requests the
 *              cloud: then image and workspace (>= s2m2_cloud_workspace_bytes(B, H, W) bytes, 4-byte aligned) are required
 *     records  (B, capacity) records of 16 bytes { float x, y, z; uint8 r, g, b, a = 255 } (16-byte aligned; the vertex layout of a binary
 *              little-endian PLY with x y z float, red green blue alpha uchar): the kept pixels of pair b in RASTER order (row-major over
 *              v, u) at records + b * capacity.  Kept pixels with rank >= capacity are not stored (the caller compares count with capacity);
 *              records beyond min(count, capacity) are left untouched.  May be NULL with capacity = 0 (count only)
 *   Two launches, no host step between them, no atomics, no waiting between blocks: the result is bit-reproducible.  Launch A: a block takes
 *   a fixed tile of whole image rows, writes the dense outputs and one count per tile into the workspace; launch B: a block sums the counts
 *   of the tiles before its own, recomputes keep, ranks its pixels with wave ballots and stores the records; the last tile of a pair stores
 *   count.  The maps are read with 16-byte loads whenever Wp % 4 == 0 and the map pointers are 16-byte aligned (any W, any crop offset).
 *   Launch plans: s2m2_cloud is NOT recorded.  Called while the calling thread records a plan (s2m2_plan_begin .. s2m2_plan_end) it fails
 *   with an error and launches nothing, so that it can never be silently missing from a plan or an engine file: the stage runs after
 *   s2m2_plan_run / s2m2_engine_run on the same stream.  Safe under stream capture (hipGraph).
 *   Errors (before any device call): null descriptor / maps / missing image or workspace, no output requested, non-positive extents, H > Hp,
 *   W > Wp, non-positive fx, fy or depth_scale, negative capacity, records NULL with capacity > 0, unknown image dtype.
 */
typedef struct s2m2_cloud_desc {
    const float* disp;
    const float* occ;
    const float* conf;
    const void* image;
    float* depth;
    unsigned char* mask;
    void* records;
    int32_t* count;
    void* workspace;
    int B, H, W, Hp, Wp;
    int image_dtype;
    int unfiltered;
    long long capacity;        /* records per pair */
    double fx, fy, cx, cy;
    double baseline, doffs;
    double depth_scale, depth_trunc;
    double conf_min, occ_min;
} s2m2_cloud_desc;
size_t s2m2_cloud_workspace_bytes(int B, int H, int W);     /* 0: bad extents */
int s2m2_cloud(const s2m2_cloud_desc* desc, void* stream);

/*
 * K16 -- the rectifier in front of the forward: undistort + rectify + bilinear resample of raw sensor images, one launch for a whole population
 *   of rectifications of one raw pair (online calibration: every candidate rotation correction is one record pair).  Replaces the host-side
 *   cv2.initUndistortRectifyMap + cv2.remap(INTER_LINEAR, BORDER_CONSTANT, 0) of the reference (src/s2m2/core/utils/calib_utils.py:354-360,
 *   image_utils.py:108-136) by their documented behaviour.
 *     src[0..n_src-1]  one or two raw images of Hs x Ws pixels, 3 channels, values in [0,255]: src_format S2M2_RECTIFY_SRC_U8_HWC (uint8,
 *                      (Hs,Ws,3) interleaved as image readers deliver it), _U8_CHW (uint8 (3,Hs,Ws) planar) or _F32_CHW (fp32 planar)
 *     records          n_img records of S2M2_RECTIFY_RECORD_FLOATS fp32 in DEVICE memory (not kernel arguments: a captured hipGraph is replayed
 *                      for the next population by rewriting this buffer only), fields at the S2M2_RECTIFY_REC_* offsets:
 *                        SRC   index of the source image as a float (0 or 1; the kernel clamps it to [0, n_src-1])
 *                        IR    iR = inv(P[:, :3] . R_rect), 9 values row-major
 *                        FX, FY, CX, CY   of the raw camera;   K1, K2, P1, P2, K3   its distortion (OpenCV order)
 *     out              (n_img, 3, Hd, Wd) planar, out_dtype S2M2_F32 or 2 (uint8) -- what S2M2.forward, s2m2_image_pad and s2m2_cloud take
 *     maps             optional (n_img, 2, Hd, Wd) fp32: mapx, mapy of every output pixel (tests, debugging)
 *   per output pixel (u, v), all in fp32 -- what cv2.initUndistortRectifyMap documents:
 *     [X Y W] = iR . [u v 1];  x = X/W;  y = Y/W;  r2 = x*x + y*y;  kr = 1 + k1 r2 + k2 r2^2 + k3 r2^3
 *     mapx = fx (x kr + 2 p1 x y + p2 (r2 + 2 x^2)) + cx;      mapy = fy (y kr + p1 (r2 + 2 y^2) + 2 p2 x y) + cy
 *   then bilinear interpolation between the four taps around (mapx, mapy); taps outside the source contribute 0.  `round` != 0 rounds the
 *   result to the nearest integer level (ties to even; the reference feeds the model uint8 images); uint8 output is always rounded and clamped.
 *   DEVIATION from cv2.remap, documented and not imitated: OpenCV quantises the coordinates to 1/32 px and interpolates uint8 images with
 *   15-bit fixed-point weights; this stage interpolates at the full fp32 coordinate.  The two differ by at most one grey level per 1/32 px of
 *   local gradient (levels per pixel).
 *   One launch, no atomics, no workspace, deterministic (every output element is written by one thread, from its own reads only).  Every lane
 *   owns four consecutive output pixels of a row (16-byte plane stores when Wd % 4 == 0 and out / maps are 16-byte aligned; any Wd otherwise).
 *   `order`: S2M2_RECTIFY_ORDER_SAMPLE (consecutive blocks are the same output tile of consecutive records, so that the blocks reading one
 *   source region run together; the default) or S2M2_RECTIFY_ORDER_TILE (all tiles of a record, then the next record); same result.
 *   Launch plans: s2m2_rectify is NOT recorded.  Called while the calling thread records a plan it fails with an error and launches nothing;
 *   the stage is not part of engine files: it runs before s2m2_plan_run / s2m2_engine_run on the same stream.  Safe under stream capture.
 *   Errors (before any device call): null descriptor / records, no output requested, null source with out requested, n_src not 1 or 2,
 *   non-positive n_img or extents, extents too large, unknown src_format / out_dtype / order, misaligned records / out / maps / fp32 source.
 */
enum { S2M2_RECTIFY_SRC_U8_HWC = 0, S2M2_RECTIFY_SRC_U8_CHW = 1, S2M2_RECTIFY_SRC_F32_CHW = 2 };
enum { S2M2_RECTIFY_ORDER_SAMPLE = 0, S2M2_RECTIFY_ORDER_TILE = 1 };
enum {
    S2M2_RECTIFY_REC_SRC = 0,
    S2M2_RECTIFY_REC_IR = 1,
    S2M2_RECTIFY_REC_FX = 10, S2M2_RECTIFY_REC_FY = 11, S2M2_RECTIFY_REC_CX = 12, S2M2_RECTIFY_REC_CY = 13,
    S2M2_RECTIFY_REC_K1 = 14, S2M2_RECTIFY_REC_K2 = 15, S2M2_RECTIFY_REC_P1 = 16, S2M2_RECTIFY_REC_P2 = 17, S2M2_RECTIFY_REC_K3 = 18,
    S2M2_RECTIFY_RECORD_FLOATS = 20          /* the record stride: 80 bytes, 19 used */
};
typedef struct s2m2_rectify_desc {
    const void* src[2];
    const float* records;
    void* out;                 /* may be NULL when maps is not */
    float* maps;               /* may be NULL */
    int n_src, n_img;
    int Hs, Ws;                /* source extents */
    int Hd, Wd;                /* output extents */
    int src_format;
    int out_dtype;             /* S2M2_F32 or 2 (uint8) */
    int round;
    int order;
} s2m2_rectify_desc;
int s2m2_rectify(const s2m2_rectify_desc* desc, void* stream);

/*
 * K18 -- the evaluation stage behind the forward: disparity error statistics against ground truth, on the device.  The reference has no such
 *   code (its numbers come from benchmark servers); the semantics are defined here and pinned by the numpy oracle of tests/eval_oracle.py.
 *   Every output is an integer, so that the result does not depend on the order of any sum.
 *     disp, occ, conf  (B,1,Hp,Wp) fp32: the padded maps as S2M2.forward / s2m2_engine_run return them; occ and conf come together or not at all
 *     gt               (B,1,H,W) fp32 ground-truth disparity, UNPADDED.  The crop of image_crop is fused as in K15: GT pixel (v,u) reads map
 *                      pixel (v + (Hp-H)/2, u + (Wp-W)/2)
 *     region           (B,1,H,W) uint8 or NULL: a pixel takes part only where region != 0 (the non-occluded mask of a benchmark)
 *   per pixel, all in fp32:
 *     in_region = region == NULL || region != 0;       evaluated = in_region && isfinite(gt) && gt > gt_min
 *     e = disp - gt;   a = |e|;   finite = isfinite(disp)
 *     a prediction that is not finite is bad at every threshold and in D1, is counted in n_nonfinite, and takes no part in the sums, in the
 *     histogram or in the sums of the confidence table
 *     q = (u64) rint(min(a, 1024) * 65536);      s = (u64) rint(min(e * e, 1048576) * 4096)         (round half to even)
 *       both scalings are exact multiplications by a power of two, so float32 arithmetic on the host reproduces q and s bit for bit.
 *       q <= 2^26 and s <= 2^32: extents are limited to H * W < 2^31 pixels per pair, so a pair's sums stay below 2^57 and 2^63 and fit in
 *       64 bits (2^23 pixels, more than any benchmark image, give 2^49 and 2^55)
 *     bad[t] = !finite || a > thr[t]             (strict; t < nthr)
 *     d1     = !finite || (a > d1_abs && a > d1_rel * |gt|)                                         (KITTI: 3 px and 0.05)
 *     hbin   = min(1024, (int) floor(a * 64))    (bins of 1/64 px over [0,16), bin 1024 = everything from 16 px on)
 *     cbin   = clamp((int) floor(conf * 64), 0, 63), a NaN confidence -> 0
 *     kept   = conf > conf_min && occ > occ_min  (the rule of K15; false without occ / conf)
 *   stats: one block of S2M2_EVAL_WORDS 64-bit words per pair:
 *     ALL   at S2M2_EVAL_ALL:  the S2M2_EVAL_BLOCK_WORDS words  N_REGION (pixels in_region), N_EVAL (evaluated), N_NONFINITE (evaluated, not
 *           finite), SUM_ABS_Q (sum of q), SUM_SQ_Q (sum of s), D1_BAD, BAD + t (t < 8)
 *     KEPT  at S2M2_EVAL_KEPT: the same words over the pixels that are also kept (N_REGION: in_region && kept, N_EVAL: evaluated && kept, ...)
 *     HIST  at S2M2_EVAL_HIST: S2M2_EVAL_HIST_BINS counts of hbin over the evaluated finite pixels
 *     CONF  at S2M2_EVAL_CONF: S2M2_EVAL_CONF_BINS rows of S2M2_EVAL_CONF_ROW_WORDS words, row cbin = COUNT (evaluated pixels of the bin),
 *           SUM_ABS_Q (over its finite ones), BAD + t
 *   EVERY word is written by every call: threshold slots t >= nthr as 0, KEPT and CONF as 0 without occ / conf.
 *   Two launches, no host step between them, no global atomics, no waiting between blocks, no dependence on what workspace or stats held
 *   before.  Launch A: a block takes a fixed tile of s2m2_eval_tile_rows(H, W) whole rows of one pair, counts in registers and in LDS (integer
 *   adds: order independent; sums that can pass 2^32 inside a tile are carried in 64 bits) and stores one partial block per tile
 *   into the workspace; launch B sums the partial blocks of each pair into stats.  Integer sums of fixed tiles: bit-reproducible.  The maps
 *   are read with 16-byte loads whenever Wp % 4 == 0 and the map pointers are 16-byte aligned, gt and region with 16- and 4-byte loads where
 *   a group of four pixels is aligned and gt is 16-byte (region 4-byte) aligned; per pixel otherwise (any W, any crop offset).
 *   Launch plans: s2m2_disp_eval is NOT recorded.  Called while the calling thread records a plan it fails with an error and launches nothing;
 *   the stage runs after s2m2_plan_run / s2m2_engine_run on the same stream.  Safe under stream capture (hipGraph).
 *   Errors (before any device call): null descriptor / disp / gt / stats / workspace, exactly one of occ and conf, non-positive extents,
 *   H > Hp, W > Wp, extents too large, nthr outside 0..8, thresholds not strictly increasing or not > 0 (or not finite), d1_abs / d1_rel /
 *   conf_min / occ_min not finite, gt_min NaN (-inf is allowed: every finite gt is valid), misaligned pointers.
 */
#define S2M2_EVAL_MAX_THR   8
#define S2M2_EVAL_HIST_BINS 1025      /* 1024 bins of 1/64 px over [0,16) + one overflow bin */
#define S2M2_EVAL_CONF_BINS 64
enum {
    S2M2_EVAL_N_REGION = 0, S2M2_EVAL_N_EVAL = 1, S2M2_EVAL_N_NONFINITE = 2, S2M2_EVAL_SUM_ABS_Q = 3, S2M2_EVAL_SUM_SQ_Q = 4,
    S2M2_EVAL_D1_BAD = 5, S2M2_EVAL_BAD = 6,
    S2M2_EVAL_BLOCK_WORDS = 14,              /* 6 + S2M2_EVAL_MAX_THR */
    S2M2_EVAL_CONF_COUNT = 0, S2M2_EVAL_CONF_SUM_ABS_Q = 1, S2M2_EVAL_CONF_BAD = 2,
    S2M2_EVAL_CONF_ROW_WORDS = 10,           /* 2 + S2M2_EVAL_MAX_THR */
    S2M2_EVAL_ALL = 0,
    S2M2_EVAL_KEPT = 14,
    S2M2_EVAL_HIST = 28,
    S2M2_EVAL_CONF = 1053,                   /* S2M2_EVAL_HIST + S2M2_EVAL_HIST_BINS */
    S2M2_EVAL_WORDS = 1693                   /* S2M2_EVAL_CONF + S2M2_EVAL_CONF_BINS * S2M2_EVAL_CONF_ROW_WORDS */
};
typedef struct s2m2_eval_desc {
    const float* disp;            /* (B,1,Hp,Wp) fp32, padded, as forward / s2m2_engine_run return it */
    const float* occ;             /* (B,1,Hp,Wp) or NULL */
    const float* conf;            /* (B,1,Hp,Wp) or NULL; occ and conf come together */
    const float* gt;              /* (B,1,H,W) fp32, UNPADDED ground-truth disparity */
    const unsigned char* region;  /* (B,1,H,W) uint8 or NULL: a pixel is evaluated only where region != 0 */
    void* workspace;              /* >= s2m2_eval_workspace_bytes(B,H,W), 8-byte aligned */
    unsigned long long* stats;    /* (B, S2M2_EVAL_WORDS) */
    int B, H, W, Hp, Wp;
    int nthr;                     /* 0 .. S2M2_EVAL_MAX_THR */
    float thr[S2M2_EVAL_MAX_THR]; /* bad-pixel thresholds in px, strictly increasing, > 0 */
    float d1_abs, d1_rel;         /* D1: |e| > d1_abs && |e| > d1_rel * |gt|   (KITTI: 3, 0.05) */
    float gt_min;                 /* gt is valid iff isfinite(gt) && gt > gt_min  (Middlebury / ETH3D: inf = invalid; KITTI: 0 = invalid) */
    float conf_min, occ_min;      /* the "kept" set: conf > conf_min && occ > occ_min (K15's rule) */
} s2m2_eval_desc;
size_t s2m2_eval_workspace_bytes(int B, int H, int W);      /* 0: bad extents */
int s2m2_eval_tile_rows(int H, int W);                      /* image rows of one tile of launch A; 0: bad extents */
int s2m2_disp_eval(const s2m2_eval_desc* desc, void* stream);

/*
 * K20 -- the surface mesh behind the 3D stage: K15's point cloud plus the triangles that connect neighbouring pixels, on the device.  The
 *   reference's demos stop at open3d point clouds (demo/visualize_3d_middlebury.py:32-52,97-107, demo/visualize_3d_booster.py); like K18 this
 *   stage has no counterpart there: the semantics are defined here and pinned by the numpy oracle of tests/mesh_oracle.py.
 *   `cloud` holds exactly the fields of s2m2_cloud, with their meaning: the padded maps, the unpadded image, the fused crop, camera and filter
 *   parameters, depth, mask, records, count, capacity, workspace.  keep, z, x, y and the colour bytes of a pixel are K15's, formula for formula.
 *   Vertices: the vertices of pair b are its kept pixels in raster order.  records and count are BYTE-IDENTICAL to what s2m2_cloud writes for
 *     the same descriptor fields (both kernels compile the same device functions).  Every kept pixel is a vertex, also one no face references.
 *   Edges: with d the value of the disp map at a pixel (the map's own value, not the filter's -1), two pixels p, q are JOINED iff
 *       keep(p) && keep(q) && fabsf(d_p - d_q) <= (float)max_jump
 *     one fp32 subtraction: exact, and contraction cannot touch it.  A comparison with NaN is false (inf - inf is NaN: not joined).  max_jump
 *     is in full-resolution pixels.
 *   Faces: every quad with top-left pixel (v,u), 0 <= v < H-1, 0 <= u < W-1, and corners a=(v,u), b=(v,u+1), c=(v+1,u), e=(v+1,u+1):
 *     all four kept:  if fabsf(d_a - d_e) <= fabsf(d_b - d_c) (a tie goes this way; false with a NaN) the diagonal is a-e and the candidates
 *                     are (a,c,e) then (a,e,b); otherwise the diagonal is b-c and the candidates are (a,c,b) then (b,c,e)
 *     exactly three kept: one candidate, the triangle of those three in the winding above: e missing (a,c,b), a missing (b,c,e), b missing
 *                     (a,c,e), c missing (a,e,b)
 *     fewer than three kept: none
 *     A candidate is emitted iff all three of its edges are joined.  All listed windings face the camera: the normal points towards -z in the
 *     camera frame (x right, y down).  Faces of a pair are stored in raster order of their quad, within a quad in the order listed; a face is
 *     three int32 vertex ranks (indices into the pair's records).
 *   outputs, beyond K15's depth, mask, records and count (unchanged in meaning):
 *     face_count (B) int32: the number of faces of every pair -- ALWAYS the true number, also above face_capacity.  Non-NULL requests the mesh
 *                and requires count, image and workspace (>= s2m2_mesh_workspace_bytes(B, H, W) bytes, 4-byte aligned).  NULL: the call is
 *                s2m2_cloud(&desc->cloud, stream) and faces / index are ignored
 *     faces      (B, face_capacity, 3) int32 at faces + b * face_capacity * 3.  Faces with rank >= face_capacity are not stored; memory beyond
 *                min(face_count, face_capacity) faces is left untouched.  May be NULL with face_capacity = 0.  The indices are true vertex
 *                ranks even when count > capacity (they then reference vertices that were not stored: the caller compares)
 *     index      optional (B,1,H,W) int32: the vertex rank of a kept pixel, -1 otherwise
 *   Three launches, no host step, no atomics, no waiting between blocks: bit-reproducible.  Launch A: a block takes a fixed tile of
 *   s2m2_mesh_tile_rows(H, W) whole image rows and reads one halo row below it, writes the dense outputs, one vertex count and one face count
 *   per tile into the workspace.  Launch B: K15's scatter, which also stores the rank of every pixel into the dense rank map (index, or the
 *   workspace).  Launch C: a block sums the face counts of the tiles before its own, applies the face rule again to disp and the rank map,
 *   ranks the two candidate slots of every quad with wave ballots and stores each face as one 12-byte record: ranks run by lane, then by
 *   quad and slot inside a lane, so a thread writes its up to eight faces back to back and the faces of a wave's step fill one contiguous
 *   range (as K15's records do).  Thread -> pixel map and 16-byte map loads as in K15.
 *   Launch plans: s2m2_mesh is NOT recorded.  Called while the calling thread records a plan it fails with an error and launches nothing; the
 *   stage runs after s2m2_plan_run / s2m2_engine_run on the same stream.  Safe under stream capture (hipGraph).
 *   Errors (before any device call): everything s2m2_cloud checks, face_count without count, H * W >= 2^30, negative face_capacity, faces NULL
 *   with face_capacity > 0, faces / face_count / index not 4-byte aligned, max_jump negative or NaN (+inf is allowed: every kept pair is joined).
 */
typedef struct s2m2_mesh_desc {
    s2m2_cloud_desc cloud;
    void* faces;
    int32_t* face_count;
    int32_t* index;
    long long face_capacity;   /* faces per pair */
    double max_jump;
} s2m2_mesh_desc;
size_t s2m2_mesh_workspace_bytes(int B, int H, int W);      /* 0: bad extents */
int s2m2_mesh_tile_rows(int H, int W);                      /* image rows of one tile of all three launches; 0: bad extents */
int s2m2_mesh(const s2m2_mesh_desc* desc, void* stream);

/*
 * K21 -- registration of the depth map to a second camera: a z-buffered forward warp of the kept pixels of the rectified left view into a
 *   target camera (the colour camera of a rig, the right view, a virtual view), on the device.  Like K18 and K20 it has no counterpart in the
 *   reference: the semantics are defined here and pinned by the numpy oracle of tests/register_oracle.py.  Still S2M2_ABI_VERSION 800: the
 *   entry points are added, nothing changes in place.
 *   `cloud` holds the INPUT fields of s2m2_cloud, with their meaning: the padded maps, the unpadded image (only needed with image_t), the fused
 *   crop, camera and filter parameters.  Its output fields (depth, mask, records, count, capacity, workspace) are IGNORED.
 *   per kept source pixel (v,u), all in fp32, every operation ONE IEEE rounding, nothing fused into a multiply-add:
 *     keep, z as in K15 (the same device function);   x = ((float)u - cx) * z / fx;   y = ((float)v - cy) * z / fy
 *     X = ((r00*x + r01*y) + r02*z) + tx;   Y = ((r10*x + r11*y) + r12*z) + ty;   Z = ((r20*x + r21*y) + r22*z) + tz
 *                                            (R row-major, source camera -> target camera; t in the unit of z; R, t and the target
 *                                            intrinsics are converted to fp32 once on the host)
 *     accepted iff Z > 0 and Z is finite
 *     up = (fx_t * X) / Z + cx_t;            vp = (fy_t * Y) / Z + cy_t
 *     c = (splat - 2) / 2  (-0.5, 0, 0.5 or 1: exact);   fu = floorf(up - c);   fv = floorf(vp - c)
 *     discarded unless fu >= -splat && fu < Wt && fv >= -splat && fv < Ht  (float comparisons, before any conversion to int: a NaN discards)
 *     footprint: the target pixels (fv + dy, fu + dx), 0 <= dx, dy < splat, those inside the target image.  splat 1 is the nearest target
 *     pixel, splat 2 the four target pixels nearest to the projected point
 *     key = ((uint64)bits(Z) << 32) | (uint32)(v * W + u)
 *   A target pixel keeps the MINIMUM key of all footprints that cover it: the nearest Z, and on exactly equal Z bits the lowest source index.
 *   outputs, each optional (NULL), at least one:
 *     depth_t  (B,1,Ht,Wt) fp32: Z (in the TARGET camera) of the winner, 0 at a hole (a target pixel that no footprint covers)
 *     index_t  (B,1,Ht,Wt) int32: the winner's source pixel v * W + u, -1 at a hole
 *     image_t  (B,3,Ht,Wt) planar uint8: the winner's colour (K15's byte rule), 0 at a hole; requires cloud.image
 *     visible  (B,1,H,W) uint8: 1 iff the source pixel won at least one target pixel -- the geometric counterpart of the occ map
 *     count    (B) int32: the covered target pixels of every pair
 *   workspace: >= s2m2_register_workspace_bytes(B, Ht, Wt) bytes, 8-byte aligned, always required: the z-buffer, one key per target pixel.
 *   Three launches, no host step.  (A) clear: the z-buffer to all ones, count and visible to 0.  (B) splat: thread -> pixel map and 16-byte
 *   map loads of K15's launch A; one 64-bit unsigned atomic minimum without return per covered target pixel.  (C) resolve: per target pixel
 *   the key is decoded, depth_t / index_t / image_t are stored densely, visible[b, index] takes a 1 (same-value plain stores) and the block's
 *   covered pixels are added to count[b] with one integer atomic add.  A minimum and an integer sum do not depend on the order of arrival and
 *   the keys are unique: the result is bit-reproducible although this stage uses atomics.
 *   Launch plans: s2m2_register is NOT recorded.  Called while the calling thread records a plan it fails with an error and launches nothing;
 *   the stage runs after s2m2_plan_run / s2m2_engine_run on the same stream.  Safe under stream capture (hipGraph).
 *   Errors (before any device call): null descriptor; everything s2m2_cloud checks on its inputs (maps, extents, fx, fy, depth_scale, image
 *   dtype, alignment); non-positive Ht, Wt, fx_t, fy_t; splat outside 1..4; a non-finite R, t or target intrinsic (also as fp32); H * W or
 *   Ht * Wt >= 2^31; no output requested; image_t without cloud.image; a missing or misaligned workspace; depth_t, index_t or count not 4-byte
 *   aligned.
 */
typedef struct s2m2_register_desc {
    s2m2_cloud_desc cloud;
    int Ht, Wt;                 /* target image */
    int splat;                  /* 1..4: side of the square footprint in target pixels */
    double fx_t, fy_t, cx_t, cy_t;
    double R[9];                /* row-major, source camera -> target camera */
    double t[3];                /* in the unit of z (i.e. after depth_scale) */
    float*         depth_t;
    int32_t*       index_t;
    unsigned char* image_t;
    unsigned char* visible;
    int32_t*       count;
    void*          workspace;
} s2m2_register_desc;
size_t s2m2_register_workspace_bytes(int B, int Ht, int Wt);   /* 0: bad extents */
int s2m2_register(const s2m2_register_desc* desc, void* stream);

/*
 * K22 -- connected components and speckle filter: the transitive closure of K20's "joined" relation, the size of every component, and the
 *   disparity map with the small components removed (what OpenCV's filterSpeckles does for classical stereo; the reference leaves it to open3d
 *   on the host).  Like K18, K20 and K21 it has no counterpart in the reference: the semantics are defined here and pinned by the numpy oracle
 *   of tests/segment_oracle.py.  Still S2M2_ABI_VERSION 800: the entry points are added, nothing changes in place.
 *   `cloud` holds the INPUT fields of s2m2_cloud, with their meaning, as s2m2_register takes them: the padded maps, H, W, Hp, Wp (fused crop),
 *   camera and filter parameters, unfiltered.  image is not read.  Its output fields (depth, mask, records, count, capacity, workspace) are
 *   IGNORED.
 *   keep of a pixel is K15's, formula for formula (the same device function).  d is the value of the disp map at the pixel (the map's own
 *   value, not the filter's -1).  A NaN or infinite disparity is never kept (K15's z is 0 for it), so d is finite wherever the rule is applied.
 *   Two pixels p, q that are neighbours in a row (left / right) or in a column (up / down) are JOINED iff
 *       keep(p) && keep(q) && fabsf(d_p - d_q) <= (float)max_jump
 *     K20's rule on the 4-neighbourhood: one fp32 subtraction, exact.  Diagonal neighbours are not joined by themselves.
 *   A COMPONENT is a class of the transitive closure of "joined" over the kept pixels of ONE pair; components never cross pairs.  A kept
 *   pixel with no joined neighbour is a component of size 1.
 *   outputs, each optional (NULL), at least one:
 *     label    (B,1,H,W) int32: for a kept pixel the raster index v * W + u of the FIRST pixel (smallest raster index) of its component; -1
 *              for a pixel that is not kept
 *     size     (B,1,H,W) int32: the number of pixels of the pixel's component; 0 where not kept
 *     mask     (B,1,H,W) uint8: survive = keep && size >= min_size
 *     disp_out (B,1,Hp,Wp) fp32, PADDED geometry: the disp map's own value where survive, -1.0f everywhere else, the border outside the crop
 *              included.  Fed to s2m2_cloud / s2m2_mesh / s2m2_register with unfiltered = 1 it yields exactly the surviving pixels with their
 *              z WHENEVER K15 itself drops d <= 0, that is whenever 1e9f / depth_scale >= depth_trunc; with depth_trunc <= 0 (1e9) K15 keeps
 *              d <= 0 at z = 1e9f / depth_scale as the reference's formula does, the removed pixels included.  Must not alias cloud.disp
 *     stats    (B,4) int32: kept pixels, components, surviving pixels, surviving components of every pair
 *   workspace: >= s2m2_segment_workspace_bytes(B, H, W) bytes, 4-byte aligned, always required: two int32 planes (parent links, sizes at the
 *   roots).  Nothing depends on what it or the outputs held before.
 *   Four launches (three where a pair is a single tile: a function of the extents, not of the data), no host step, no waiting between blocks.
 *   (A) local: a block takes a tile of s2m2_segment_tile_rows x s2m2_segment_tile_cols pixels -- tile column tx spans the image columns
 *   [tx * tile_cols - s, (tx + 1) * tile_cols - s) with s = ((Wp - W) / 2) & 3, tile row ty the rows [ty * tile_rows, (ty + 1) * tile_rows) --,
 *   evaluates keep, resolves the tile's components by union-find in LDS, counts their pixels there, and stores every pixel's root as a global
 *   raster index and every root's count.  (B) border: one thread per pixel of a tile's right column or bottom row unites it with its joined
 *   neighbour across the border (int32 atomic minima on the link array).  (C) flatten: every link is replaced by its root, and the count of a
 *   tile's root moves to the component's root (one int32 atomic add per tile and component).  (D) outputs: a walk over the padded geometry.  A link only ever moves to a smaller index of its component, so every
 *   loop is bounded by an index, and the root of a component is its smallest raster index whatever the order of arrival; sizes and counts are
 *   integer sums: the result is bit-reproducible although this stage uses atomics.
 *   Launch plans: s2m2_segment is NOT recorded.  Called while the calling thread records a plan it fails with an error and launches nothing;
 *   the stage runs after s2m2_plan_run / s2m2_engine_run on the same stream.  Safe under stream capture (hipGraph).
 *   Errors (before any device call): null descriptor; everything s2m2_cloud checks on its inputs (maps, extents, fx, fy, depth_scale, image
 *   dtype, alignment); H * W >= 2^30; no output requested; a missing or misaligned workspace; label, size, disp_out or stats not 4-byte aligned
 *   (mask: any alignment); disp_out == cloud.disp; max_jump negative or NaN (+inf is allowed: every kept pair of neighbours is joined);
 *   min_size < 1 or > 2^30.
 */
typedef struct s2m2_segment_desc {
    s2m2_cloud_desc cloud;
    int32_t*       label;
    int32_t*       size;
    unsigned char* mask;
    float*         disp_out;
    int32_t*       stats;
    void*          workspace;
    double         max_jump;   /* px, >= 0 */
    long long      min_size;   /* >= 1; 1 removes nothing (labels and sizes only) */
} s2m2_segment_desc;
size_t s2m2_segment_workspace_bytes(int B, int H, int W);   /* 0: bad extents */
int s2m2_segment_tile_rows(int H, int W);                   /* the tile of launch A (at most H), so that tests can aim at its borders; 0: bad extents */
int s2m2_segment_tile_cols(int H, int W);                   /* ... (at most W) */
int s2m2_segment(const s2m2_segment_desc* desc, void* stream);

/*
 * K23 -- voxel-grid downsampling of K15's point cloud: one record per occupied voxel, the centroid and the mean colour of the kept points in it
 *   (what open3d's voxel_down_sample and PCL's VoxelGrid do on the host).  Like K18 and K20 to K22 it has no counterpart in the reference: the
 *   semantics are defined here and pinned by the numpy oracle of tests/voxel_oracle.py.  Still S2M2_ABI_VERSION 800: the entry points are
 *   added, nothing changes in place.
 *   `cloud` holds the INPUT fields of s2m2_cloud, with their meaning, as s2m2_segment takes them: the padded maps, the unpadded image (always
 *   required here), H, W, Hp, Wp (fused crop), camera and filter parameters, unfiltered.  Its output fields are IGNORED.
 *   Which points.  keep, z, x, y and the colour bytes of a pixel are K15's, formula for formula (the same device functions).
 *   Quantisation.  vs = (float)voxel_size, in the units of z; q = vs / 1024.0f (exact).  Per axis X = rintf(x / q): one fp32 division, one
 *     round-to-nearest-even, in float; Y and Z likewise.  A kept point is IN RANGE iff fabsf(X), fabsf(Y) and fabsf(Z) are all < 2^30; kept
 *     points out of range are dropped and counted (with depth_trunc <= 0 K15 keeps d <= 0 at z = 1e9f / depth_scale: such points usually land
 *     here).  With the integer X: the voxel index ix = X >> 10 (floor, also for negative X) and the local offset lx = X & 1023; iy, iz, ly, lz
 *     likewise.  A voxel is the triple (ix, iy, iz), each in [-2^20, 2^20).  Everything behind the one division is integer arithmetic.
 *   Per voxel, integer aggregates over its points: n (int32), the sums of lx, ly, lz and of the colour bytes r, g, b (64 bits each), and
 *     first, the smallest raster index v * W + u of its points.
 *   Record of a voxel (16 bytes, K15's format):
 *       x = (float)(((double)ix * 1024.0 + (double)sum_lx / (double)n) * (double)q);    y, z likewise
 *       colour byte = (2 * sum + n) / (2 * n) in integers (the mean rounded to nearest, halves up);    a = 255
 *     The records of a pair are stored in ascending `first`: the raster order of the voxels' first points.  A pixel is its voxel's LEADER iff
 *     its raster index equals first.
 *   outputs, each optional (NULL), at least one:
 *     records  (B, capacity) 16-byte records (16-byte aligned) at records + b * capacity
 *     weights  (B, capacity) int32: n of each record
 *     count    (B) int32: the number of voxels in the table -- the true number also above `capacity`; records and weights of rank >= capacity are
 *              not stored and the rest of both buffers is left untouched
 *     index    (B,1,H,W) int32: the record rank of the pixel's voxel (the true rank, also >= capacity); -1 where the pixel is not kept or was
 *              dropped.  One more launch, only when requested
 *     stats    (B,4) int32: kept points, points dropped out of range, points dropped because the table was full, voxels
 *   Table.  max_voxels (per pair, 1 .. 2^29) sizes an open-addressing hash table of `slots` slots of 64 bytes per pair in the workspace, slots =
 *     the smallest power of two >= 2 * max_voxels.  workspace: >= s2m2_voxel_workspace_bytes(B, H, W, max_voxels) bytes, 16-byte aligned: the
 *     tables, an int32 plane (B,H,W) with every pixel's slot, the tile counts and the counters.  Nothing depends on what it held before: the
 *     call clears what it needs.  A new voxel is claimed by the one thread that wins its slot, and only that thread asks the pair's occupancy
 *     counter for room: a pair with at most max_voxels distinct voxels never loses a point (stats[2] == 0), however the insertions race, and
 *     uses at most max_voxels slots, so its load stays <= 1/2.  If a pair has more than max_voxels distinct voxels, the winner that finds no
 *     room sets the pair's full flag, and it and every later point that meets an empty slot give up and are counted in stats[2]; the
 *     records, weights and index of THAT pair are unspecified (which points were dropped depends on arrival) and count <= slots.  Every probe
 *     loop is bounded by `slots` whatever the load.
 *   Launches: clear the table; insert (key compare-and-swap with linear probing from s2m2_voxel_home_slot, int32 / int64 atomic adds, an
 *     atomic minimum for first; runs of neighbouring pixels in one voxel are summed in registers and across the lanes of a wave first and
 *     insert once); count the leaders per raster tile; rank them and store; index when requested.  No host step, no synchronisation, no
 *     waiting between blocks.  Integer sums and minima do not depend on the order or grouping of their operands, the record is a function of
 *     them alone, and the order of the records is the raster order of the leaders: the outputs are bit-reproducible although this stage uses
 *     atomics and although the slot a voxel lands in depends on arrival.
 *   Launch plans: s2m2_voxel is NOT recorded.  Called while the calling thread records a plan it fails with an error and launches nothing;
 *   the stage runs after s2m2_plan_run / s2m2_engine_run on the same stream.  Safe under stream capture (hipGraph).
 *   Errors (before any device call): null descriptor; everything s2m2_cloud checks on its inputs (maps, extents, fx, fy, depth_scale, image
 *   dtype, alignment); a null image; voxel_size not finite or <= 0 in fp32; max_voxels < 1 or > 2^29 (the slot count would reach 2^31); no
 *   output requested; negative capacity; records and weights both NULL with capacity > 0; records not 16-byte aligned; a missing workspace or
 *   one not 16-byte aligned; weights, count, index or stats not 4-byte aligned.
 */
typedef struct s2m2_voxel_desc {
    s2m2_cloud_desc cloud;
    void*          records;
    int32_t*       weights;
    int32_t*       count;
    int32_t*       index;
    int32_t*       stats;
    void*          workspace;
    double         voxel_size; /* > 0, in the units of z */
    long long      max_voxels; /* per pair, 1 .. 2^29 */
    long long      capacity;   /* records (and weights) per pair */
} s2m2_voxel_desc;
size_t s2m2_voxel_workspace_bytes(int B, int H, int W, long long max_voxels);   /* 0: bad extents or max_voxels */
int s2m2_voxel_tile_rows(int H, int W);                    /* rows of a raster tile (K15's, at most H), so that tests can aim at its borders; 0: bad extents */
/* the slot where the probe chain of voxel (ix, iy, iz) starts in a table of `slots` slots (a power of two, 2 .. 2^30), so that tests can aim
 * at probe chains; host code; -1: bad arguments */
long long s2m2_voxel_home_slot(int ix, int iy, int iz, long long slots);
int s2m2_voxel(const s2m2_voxel_desc* desc, void* stream);

/*
 * K24 -- depth maps of a moving rig fused into a truncated signed distance (TSDF) volume, and the surface of that volume as a point cloud (what
 *   open3d's TSDFVolume.integrate / extract_point_cloud do on the host).  The first stage that carries state from one pair to the next.  Like
 *   K18 and K20 to K23 it has no counterpart in the reference: the semantics are defined here and pinned by the numpy oracle of
 *   tests/tsdf_oracle.py.  Still S2M2_ABI_VERSION 800: the entry points are added, nothing changes in place.
 *   The volume: a dense grid of Nx * Ny * Nz voxels in caller-owned device memory, 16 bytes per voxel, 16-byte aligned:
 *       { float tsdf; int32 weight; uint16 r, g, b, pad; }        voxel (i, j, k) at lin = (k * Ny + j) * Nx + i;   Nx * Ny * Nz < 2^29
 *     r, g, b are the colour as fixed-point 8.8 values; pad is kept as it is.  An all-zero buffer is an empty volume; there is no clear entry
 *     point (hipMemsetAsync is the reset).  origin is the centre of voxel (0,0,0) in the world frame; voxel_size and trunc are in the unit of
 *     z (i.e. after depth_scale).
 *   s2m2_tsdf_integrate.  `cloud` holds the INPUT fields of s2m2_cloud, with their meaning, as s2m2_register takes them: the B padded maps,
 *     the unpadded image (always required here), H, W, Hp, Wp (fused crop), camera and filter parameters, unfiltered.  Its output fields are
 *     IGNORED.  poses is a DEVICE buffer (B, 12) fp32, row-major [R | t] per pair: p_cam = R p_world + t (t in the unit of z).  A captured graph
 *     serves the next frames once that buffer (and the maps) are rewritten; no host pointer reaches a kernel.  The intrinsics, origin,
 *     voxel_size and trunc are converted to fp32 once on the host.
 *     per voxel (i, j, k), for the pairs b = 0 .. B-1 of the call in that order, all in fp32, every operation ONE IEEE rounding, nothing fused
 *     into a multiply-add:
 *       x = ox + (float)i * vs;   y = oy + (float)j * vs;   z = oz + (float)k * vs
 *       X = ((r00*x + r01*y) + r02*z) + tx;   Y = ((r10*x + r11*y) + r12*z) + ty;   Z = ((r20*x + r21*y) + r22*z) + tz        (K21's form)
 *       skip unless Z > 0 and Z is finite
 *       up = (fx * X) / Z + cx;   vp = (fy * Y) / Z + cy;   fu = rintf(up);   fv = rintf(vp)                                  (half to even)
 *       skip unless fu >= 0 && fu < W && fv >= 0 && fv < H     (float comparisons, before any conversion to int: a NaN skips)
 *       pixel (fv, fu) of the UNPADDED image: keep, z_pix and the colour bytes are K15's (the same device functions, fused crop)
 *       skip unless keep
 *       sdf = z_pix - Z;   skip unless sdf >= -trunc;   skip if !carve && sdf > trunc
 *       d = fminf(sdf / trunc, 1.0f)
 *       Wf = (float)weight
 *       tsdf   = (tsdf * Wf + d) / (Wf + 1.0f)                                             (three roundings: mul, add, div)
 *       colour = (colour * weight + (byte << 8) + ((weight + 1) >> 1)) / (weight + 1)      per channel, unsigned 32-bit integers
 *       weight = min(weight + 1, max_weight)
 *     With weight <= 32767 a colour stays <= 65280 and the numerator below 2^32.  A voxel that no pair of the call updates is neither written
 *     nor changed, whatever its bytes were.  A voxel is read and written at most once per call, however large B is: the loop over the pairs
 *     runs inside the thread that owns the voxel.  One launch, no atomics, no workspace: bit-reproducible.
 *     Errors (before any device call): null descriptor; everything s2m2_cloud checks on its inputs (maps, extents, fx, fy, depth_scale, image
 *     dtype, alignment); a null volume, poses or image; a volume not 16-byte or poses not 4-byte aligned; non-positive dims or Nx*Ny*Nz >=
 *     2^29; voxel_size or trunc not finite or <= 0 as fp32; a non-finite origin; max_weight outside 1 .. 32767.
 *   s2m2_tsdf_extract.  A voxel is OBSERVED iff weight >= min_weight (min_weight >= 1).  For every observed voxel v0 = (i, j, k) in ascending
 *     lin, and for the axes x, y, z in that order: v1 is v0's neighbour at +1 along the axis, t0 and t1 their tsdf, and a point is emitted iff
 *     v1 is inside the grid and observed and (t0 < 0) != (t1 < 0).  Per emitted point, in fp32 with one rounding per operation:
 *       s = t0 / (t0 - t1);   the coordinate along the axis is (o_a + (float)i_a * vs) + s * vs, the other two are the centre of v0
 *       sel = fabsf(t1) < fabsf(t0) ? v1 : v0;   colour byte = (c_sel + 128) >> 8;   a = 255
 *       gradient g_b = tp - tm per axis b: tp / tm are the tsdf of sel's +b / -b neighbour where that neighbour is inside the grid and
 *       observed, t_sel otherwise.  Unnormalised; it points from the surface to free space.
 *     outputs, each optional (NULL), at least one:
 *       records    (capacity) K15's 16-byte records (16-byte aligned)
 *       gradients  (capacity, 3) fp32
 *       count      one int32: the true number of points, also above `capacity`; points of rank >= capacity are not stored and the rest of both
 *                  buffers is left untouched
 *     workspace: >= s2m2_tsdf_workspace_bytes(Nx, Ny, Nz) bytes, 4-byte aligned, always required.  Two launches as in K15, no host step, no
 *     atomics: a block counts the points of a tile of s2m2_tsdf_tile_voxels(Nx, Ny, Nz) consecutive voxels, then the blocks rank and store.
 *     Bit-reproducible.
 *     Errors (before any device call): null descriptor; a null or misaligned volume; non-positive dims or Nx*Ny*Nz >= 2^29; voxel_size not
 *     finite or <= 0 as fp32; a non-finite origin; min_weight < 1; no output requested; negative capacity; records and gradients both NULL
 *     with capacity > 0; records not 16-byte aligned; gradients or count not 4-byte aligned; a missing or misaligned workspace.
 *   Launch plans: s2m2_tsdf_integrate and s2m2_tsdf_extract are NOT recorded.  Called while the calling thread records a plan they fail with an
 *   error and launch nothing; the stage runs after s2m2_plan_run / s2m2_engine_run on the same stream.  Safe under stream capture (hipGraph).
 */
typedef struct s2m2_tsdf_desc {
    s2m2_cloud_desc cloud;
    void*          volume;     /* Nx * Ny * Nz voxels of 16 bytes, 16-byte aligned */
    const float*   poses;      /* DEVICE (B, 12) fp32: [R | t] row-major per pair, world -> camera */
    int            Nx, Ny, Nz;
    int            max_weight; /* 1 .. 32767 */
    int            carve;      /* != 0: voxels in front of the band (sdf > trunc) are updated with d = 1 */
    double         origin[3];  /* centre of voxel (0,0,0) */
    double         voxel_size; /* > 0, in the unit of z */
    double         trunc;      /* > 0, in the unit of z */
} s2m2_tsdf_desc;
typedef struct s2m2_tsdf_extract_desc {
    const void*    volume;
    void*          records;
    float*         gradients;
    int32_t*       count;
    void*          workspace;
    int            Nx, Ny, Nz;
    int            min_weight; /* >= 1 */
    long long      capacity;   /* records (and gradients) */
    double         origin[3];
    double         voxel_size;
} s2m2_tsdf_extract_desc;
size_t s2m2_tsdf_workspace_bytes(int Nx, int Ny, int Nz);   /* 0: bad dims */
int s2m2_tsdf_tile_voxels(int Nx, int Ny, int Nz);          /* consecutive voxels of one extraction tile, so that tests can aim at its borders; 0: bad dims */
int s2m2_tsdf_integrate(const s2m2_tsdf_desc* desc, void* stream);
int s2m2_tsdf_extract(const s2m2_tsdf_extract_desc* desc, void* stream);

/*
 * K25 -- the surface of K24's volume as a triangle mesh (what open3d's TSDFVolume.extract_triangle_mesh does on the host): marching cubes on
 *   the device, "K20 for the volume".  No counterpart in the reference: the semantics are defined here and pinned by the numpy oracle of
 *   tests/tsdf_mesh_oracle.py.  Still S2M2_ABI_VERSION 800: the entry points are added, nothing changes in place.
 *   Cells.  A cell is (i, j, k) with 0 <= i < Nx-1, 0 <= j < Ny-1, 0 <= k < Nz-1; its corner c = dx + 2 dy + 4 dz is voxel (i+dx, j+dy, k+dz).
 *     A cell is VALID iff all eight corners are observed (weight >= min_weight, K24's predicate).  Its case is the sum of (t_c < 0) << c, the
 *     sign predicate of K24: +0.0 and -0.0 are not negative.  A grid with an extent of 1 has no cells.
 *   Vertices.  Exactly the points of s2m2_tsdf_extract for the same volume, origin, voxel_size and min_weight: records, gradients and count are
 *     BYTE-IDENTICAL to what s2m2_tsdf_extract writes, the capacity rule included (both entry points compile the same device functions).  Every
 *     point is a vertex, also one that no face references.  Edge e = (axis a, base corner b with bit a clear) of a cell carries the vertex that
 *     K24 emits for voxel (cell + b) along axis a; its index is that point's rank.  The edges are numbered axis-major: for a in 0..2, the bases b
 *     in ascending order.  In a valid cell every sign-changing edge joins two observed voxels, so its point exists.
 *   Faces.  The valid cells are visited in ascending lin = (k * Ny + j) * Nx + i; inside a cell the triangles come in the order of the case
 *     table.  A face is three int32 vertex ranks, wound so that its normal points to free space (the positive side, where K24's gradients
 *     point).  The indices are true ranks also when count > capacity: the caller compares, as for K20.
 *   Case table.  256 cases, each a list of at most 5 triangles over the 12 edge numbers, 820 in all, GENERATED by s2m2_amd/mc_table.py
 *     (csrc/mc_table.h is its output; the oracle imports the same build_table()).  The construction: on each cube face two sign-changing edges
 *     are joined by a segment, and four (diagonal corners alike) by two segments that cut off the two NEGATIVE corners separately -- this depends
 *     on the face's four signs alone, so the two cells sharing a face agree; the segments close into loops, taken in the order of their lowest
 *     edge and oriented to the positive side; a loop is triangulated as a fan from the first apex (rotating from its lowest edge) for which no
 *     fan diagonal lies in a cube face.  The meshes are closed oriented 2-manifolds wherever the cells around the surface are valid.
 *   Degenerate input.  A tsdf of exactly zero puts several vertices on one voxel centre; the zero-area triangles that result are emitted and
 *     are part of the contract.
 *   `extract`: every field with K24's meaning; records, gradients and count are each optional, and all three may be NULL (a faces-only call).
 *     faces       (face_capacity, 3) int32, 4-byte aligned; may be NULL with face_capacity 0
 *     face_count  one int32, REQUIRED: the true number of faces, also above face_capacity; faces of rank >= face_capacity are not stored and
 *                 memory behind min(face_count, face_capacity) faces is left untouched
 *     workspace (extract.workspace): >= s2m2_tsdf_mesh_workspace_bytes(Nx, Ny, Nz) bytes, 4-byte aligned: 4 bytes per voxel (the rank map: the
 *     rank of a voxel's first point) plus 8 bytes per tile of s2m2_tsdf_tile_voxels voxels, each part rounded up to 256 bytes.
 *     face_count is an int32, so Nx*Ny*Nz <= (2^31 - 1) / 5 = 429 496 729 (tighter than K24's 2^29; 512^3 passes).
 *     Three launches, no host step, no atomics, no waiting between blocks: a block counts the points and the faces of a tile, the blocks rank
 *     and store the points (K24's store launch, which also writes the rank map), then rank and store the faces.  Bit-reproducible.
 *     Errors (before any device call): null descriptor; everything s2m2_tsdf_extract checks except "no output requested"; a null or misaligned
 *     face_count; misaligned faces; negative face_capacity; faces NULL with face_capacity > 0; the size limit above; a missing or misaligned
 *     workspace.
 *   Launch plans: s2m2_tsdf_mesh is NOT recorded.  Called while the calling thread records a plan it fails with an error and launches nothing.
 *   Safe under stream capture (hipGraph).
 */
typedef struct s2m2_tsdf_mesh_desc {
    s2m2_tsdf_extract_desc extract;   /* every field with K24's meaning; workspace >= s2m2_tsdf_mesh_workspace_bytes */
    void*          faces;             /* (face_capacity, 3) int32, 4-byte aligned; may be NULL with face_capacity 0 */
    int32_t*       face_count;        /* one int32, REQUIRED: the true number of faces, also above face_capacity */
    long long      face_capacity;
} s2m2_tsdf_mesh_desc;
size_t s2m2_tsdf_mesh_workspace_bytes(int Nx, int Ny, int Nz);   /* 0: bad dims, or more voxels than the size limit */
int s2m2_tsdf_mesh(const s2m2_tsdf_mesh_desc* desc, void* stream);

/*
 * K26 -- K24's volume ray-cast into the depth, gradient and colour maps of a camera (what open3d's RaycastingScene or KinectFusion's surface
 *   prediction do): what the volume holds, seen from a given pose, in K21's layout -- depth with 0 as the hole value, a uint8 image, a count.
 *   No counterpart in the reference: the semantics are defined here and pinned by the numpy oracle of tests/tsdf_raycast_oracle.py.  Still
 *   S2M2_ABI_VERSION 800: the entry point is added, nothing changes in place.
 *   All in fp32, every operation ONE IEEE rounding, nothing fused into a multiply-add.  fx, fy, cx, cy, origin, voxel_size (vs), z_near, z_far
 *   and step are converted to fp32 once on the host; n_steps = ceil((z_far - z_near) / step), computed on the host in double from the fp32
 *   values, is the length of the march (at most 65536).  poses is K24's DEVICE buffer (B, 12): [R | t] row-major, world -> camera; R is taken
 *   as given (nothing checks orthonormality).  Per pair b and target pixel (v, u):
 *     ray      dx = ((float)u - cx) / fx;   dy = ((float)v - cy) / fy
 *              wx = (r00*dx + r10*dy) + r20   (R^T applied to (dx, dy, 1));   wy, wz likewise with the columns 1 and 2 of R
 *              ox_w = -((r00*tx + r10*ty) + r20*tz)   (the camera centre);    oy_w, oz_w likewise
 *              a_x = (ox_w - origin_x) / vs;   b_x = wx / vs;   y and z likewise.   The position in voxel units at depth z: g = a + z * b
 *     samples  z_k = z_near + (float)k * step,   k = 0 .. n_steps-1
 *     observed f0 = floorf(g) per axis.  The sample is OBSERVED iff f0_a >= 0 && f0_a <= (float)(N_a - 2) on all three axes (float comparisons,
 *              before any conversion to int: a NaN or Inf fails them and no address is formed) and all eight corners (i0+dx, j0+dy, k0+dz) of the
 *              cell (i0, j0, k0) = f0 have weight >= min_weight (K24's predicate).  A grid with an extent of 1 has no observed sample.
 *     value    fr_a = g_a - f0_a;   trilinear along x, then y, then z, each as lo + fr * (hi - lo) (sub, mul, add): four x-lerps c00, c10, c01,
 *              c11 (index = dy, dz), two y-lerps c0, c1, one z-lerp t
 *     march    have_prev = false; for ascending k: an unobserved sample sets have_prev = false; else if have_prev && !(t_prev < 0) && (t < 0) this
 *              is the crossing (+0.0 and -0.0 are not negative: K24's sign predicate); else have_prev = true, t_prev = t, z_prev = z_k.  The
 *              first crossing ends the march; no crossing within n_steps: the pixel is a hole.
 *     hit      z_hit = z_prev + (t_prev / (t_prev - t)) * (z_k - z_prev);   the volume is sampled again at g_hit = a + z_hit * b.  Unobserved: the
 *              pixel is a HOLE (the march does not resume).  Otherwise depth = z_hit.
 *     gradient the analytic gradient of the trilinear interpolant in the hit cell, from the same eight corners: Gx from the four differences
 *              t(1,y,z) - t(0,y,z), lerped along y with fr_y, then along z with fr_z, in the same lo + fr * (hi - lo) form; Gy lerped along x,
 *              then z; Gz along x, then y.  WORLD frame, per voxel, unnormalised, pointing to free space as K24's gradients do.
 *     colour   of the corner nearest to g_hit: per axis i0 + (fr_a >= 0.5f);   byte = (c + 128) >> 8 per channel (K24's rounding)
 *   outputs, each optional (NULL), at least one; every pixel of every requested output is written, a hole as 0 / 0,0,0 / 0,0,0:
 *     depth      (B,1,Ht,Wt) fp32, z in the camera
 *     gradients  (B,3,Ht,Wt) fp32
 *     image      (B,3,Ht,Wt) uint8
 *     count      (B) int32 covered pixels: cleared on the stream by the entry point, then one atomic integer add per block.  The sum does not
 *                depend on the order, so the stage stays bit-reproducible.
 *   The kernel skips samples that a slab clip of the ray against the grid box proves to lie outside the grid; they are unobserved by the rule, so
 *   no bit of the result depends on it.  One launch plus the clear of count, no workspace, no host step.
 *   Errors (before any device call): null descriptor; everything K24 checks of a volume (null or misaligned, dims, voxel_size, origin); null or
 *   misaligned poses; no output requested; depth, gradients or count not 4-byte aligned; B, Ht or Wt <= 0 or B*Ht*Wt >= 2^31; fx or fy not
 *   finite or zero as fp32; non-finite cx or cy; min_weight < 1; z_near, z_far or step not finite or outside the ranges below as fp32;
 *   n_steps > 65536.
 *   Launch plans: s2m2_tsdf_raycast is NOT recorded.  Called while the calling thread records a plan it fails with an error and launches nothing.
 *   Safe under stream capture (hipGraph).
 */
typedef struct s2m2_tsdf_raycast_desc {
    const void*  volume;          /* K24's volume, 16-byte aligned */
    const float* poses;           /* DEVICE (B, 12) fp32 [R | t] row-major, world -> camera: K24's convention */
    float*       depth;           /* (B,1,Ht,Wt) fp32, z in the camera, 0 = hole; optional */
    float*       gradients;       /* (B,3,Ht,Wt) fp32, WORLD frame, unnormalised, 0 at holes; optional */
    uint8_t*     image;           /* (B,3,Ht,Wt) uint8, 0 at holes; optional */
    int32_t*     count;           /* (B) covered pixels; optional */
    int          B, Ht, Wt;
    int          Nx, Ny, Nz;
    int          min_weight;      /* >= 1, K24's OBSERVED predicate */
    double       fx, fy, cx, cy;  /* target camera */
    double       origin[3];
    double       voxel_size;
    double       z_near, z_far, step;  /* in the unit of z; 0 <= z_near < z_far, step > 0 */
} s2m2_tsdf_raycast_desc;
int s2m2_tsdf_raycast(const s2m2_tsdf_raycast_desc* desc, void* stream);

/*
 * K27 -- the camera tracked against K24's volume: frame-to-model point-to-plane ICP with projective data association (KinectFusion's tracking
 *   step).  The live frame is K15's maps; the model is what K26 rendered from `model_poses`: depth and the world-frame tsdf gradients.  The
 *   refined pose is written into the DEVICE pose buffer that s2m2_tsdf_integrate / s2m2_tsdf_raycast read next, so that raycast -> track ->
 *   integrate is one capturable chain without a host step.  No counterpart in the reference: the semantics are defined here and pinned by the
 *   numpy oracle of tests/tsdf_track_oracle.py.  Still S2M2_ABI_VERSION 800: the entry points are added, nothing changes in place.
 *   `cloud` holds the INPUT fields of s2m2_cloud with the meaning they have in s2m2_tsdf_desc: the B padded maps, H, W, Hp, Wp (fused crop),
 *   camera and filter parameters, unfiltered.  Its outputs are IGNORED and the image is not needed.  mfx, mfy, mcx, mcy (the model camera, which
 *   may differ from the live one) and max_dist are converted to fp32 once on the host; max_dist2 = max_dist * max_dist is formed once on the
 *   host as fp32.
 *   Per iteration it = 0 .. n_iters-1, per pair b with [R | t] = poses[b] (as the previous iteration left it) and [Rm | tm] = model_poses[b],
 *   per pixel (v, u) of the UNPADDED live image, all in fp32, every operation ONE IEEE rounding, nothing fused into a multiply-add:
 *     live     z, keep = K15's (the same device functions); skip unless keep (z > 0);   x = ((float)u - cx) * z / fx;   y = ((float)v - cy) * z / fy
 *     world    c = (x - tx, y - ty, z - tz);   p_a = (r0a*c0 + r1a*c1) + r2a*c2   for a = x, y, z  (R^T applied: K26's form)
 *     model    X = ((m00*px + m01*py) + m02*pz) + tmx;   Y, Z likewise with the rows 1 and 2 of Rm                              (K24's form)
 *              skip unless Z > 0 and Z is finite
 *              up = (mfx * X) / Z + mcx;   vp = (mfy * Y) / Z + mcy;   fu = rintf(up);   fv = rintf(vp)                           (half to even)
 *              skip unless fu >= 0 && fu < Wt && fv >= 0 && fv < Ht   (float comparisons, before any conversion to int: a NaN skips)
 *     surface  dm = model_depth[b, fv, fu];   skip unless dm > 0
 *              g = model_gradients[b, 0..2, fv, fu];   s = (gx*gx + gy*gy) + gz*gz;   skip unless s > 0 and s is finite
 *              q = sqrtf(s);   n = (gx / q, gy / q, gz / q)
 *              mx = (fu - mcx) * dm / mfx;   my = (fv - mcy) * dm / mfy;   e = (mx - tmx, my - tmy, dm - tmz)
 *              w_a = (m0a*e0 + m1a*e1) + m2a*e2                                                                                  (Rm^T applied)
 *     gate     d = w - p;   skip unless (dx*dx + dy*dy) + dz*dz <= max_dist2   (a NaN skips)
 *     row      r = (nx*dx + ny*dy) + nz*dz
 *              J = (py*nz - pz*ny,  pz*nx - px*nz,  px*ny - py*nx,  nx,  ny,  nz)
 *   Sums.  J0..J5 and r are widened to double; the 21 products Ji*Jj (i <= j), the 6 products Ji*r and r*r are exact in double, and they are
 *     accumulated in double, with an integer count, over the pixels of the pair that were not skipped.  No floating-point atomics: a thread sums
 *     its pixels, a wave its threads, a block its waves, and a fixed pass sums the per-tile partials, so the order of the additions depends on
 *     the shapes alone and the result is bit-reproducible.  Any order is within (count-1) roundings of the exact sum.
 *   Solve and update, per pair, in double:
 *     status 1 if count < min_count; else status 2 if any of the 28 sums is not finite; else Cholesky of the 6 x 6 A = sum J J^T without
 *     pivoting, status 2 at a pivot that is not > 0 (or not finite); xi = (omega, v) = A^-1 sum J r; status 2 if an entry of xi is not finite;
 *     status 3 if |omega| > max_rot or |v| > max_trans.
 *     E = I + a K + b K^2 with K = [omega]x, th = |omega|, a = sin(th) / th, b = (1 - cos(th)) / th^2 (th < 1e-4: a = 1 - th^2/6, b = 1/2 -
 *     th^2/24);   R' = R E^T, its rows re-orthonormalised (row 0 normalised, row 1 minus its part along row 0 and normalised, row 2 = row 0 x
 *     row 1);   t' = t - R' v.  Every entry is rounded to fp32 once; status 2 if one of them is not finite.  With status 0 the twelve numbers
 *     replace poses[b]; with any other status poses[b] is left as it was, byte for byte, and the remaining iterations still run (they repeat the
 *     verdict).  This moves the live points by p <- E p + v in the world.
 *   systems  optional (B, n_iters, 32) float64, 8-byte aligned; the row of (b, it): [0..20] A's upper triangle, row-major; [21..26] sum J r;
 *            [27] sum r*r; [28] count; [29] status; [30] |omega|; [31] |v| -- the norms with status 0 and 3, 0 with status 1 and 2.
 *   residual optional (B,1,H,W) fp32: r of the LAST iteration's association (computed from the pose that iteration started from); the bit
 *            pattern 0x7fc00000 at every pixel that was not kept or was skipped.  Every pixel is written.
 *   workspace: >= s2m2_tsdf_track_workspace_bytes(B, H, W) bytes, 8-byte aligned: 32 doubles per tile of K15's raster walk (whole rows, as
 *   many as fit 4096 pixels).
 *   Two launches per iteration, no host step: the blocks walk K15's tiles and write one partial each; one block per pair sums the partials,
 *   solves and updates.
 *   Errors (before any device call): null descriptor; everything s2m2_tsdf_integrate checks of its maps and camera; null or misaligned (4 bytes)
 *   poses, model_poses, model_depth, model_gradients; a null or misaligned (8 bytes) workspace; Ht or Wt <= 0 or B*Ht*Wt >= 2^31; mfx or mfy
 *   zero or not finite as fp32; non-finite mcx or mcy; max_dist, max_rot or max_trans not finite or <= 0 as fp32; min_count < 6; n_iters outside
 *   1 .. 64; systems not 8-byte aligned; residual not 4-byte aligned.
 *   Non-finite poses or maps never form an address: they end in status 1 or 2.
 *   Launch plans: s2m2_tsdf_track is NOT recorded.  Called while the calling thread records a plan it fails with an error and launches nothing.
 *   Safe under stream capture (hipGraph).
 */
typedef struct s2m2_tsdf_track_desc {
    s2m2_cloud_desc cloud;           /* the live maps: K24's meaning; outputs ignored, image not needed */
    float*       poses;              /* DEVICE (B, 12) fp32 [R | t] row-major, world -> camera: the initial guess in, the refined pose out */
    const float* model_poses;        /* DEVICE (B, 12): the poses K26 rendered the model maps from */
    const float* model_depth;        /* (B,1,Ht,Wt) fp32: K26's depth */
    const float* model_gradients;    /* (B,3,Ht,Wt) fp32: K26's gradients */
    double*      systems;            /* (B, n_iters, 32) float64; optional */
    float*       residual;           /* (B,1,H,W) fp32; optional */
    void*        workspace;          /* >= s2m2_tsdf_track_workspace_bytes(B, H, W), 8-byte aligned */
    int          Ht, Wt;             /* the model camera */
    int          min_count;          /* >= 6 */
    int          n_iters;            /* 1 .. 64 */
    double       mfx, mfy, mcx, mcy;
    double       max_dist;           /* correspondence gate, in the unit of z */
    double       max_rot, max_trans; /* per-iteration step gate: radians, unit of z */
} s2m2_tsdf_track_desc;
size_t s2m2_tsdf_track_workspace_bytes(int B, int H, int W);   /* 0: bad extents */
int s2m2_tsdf_track(const s2m2_tsdf_track_desc* desc, void* stream);

/*
 * K28 -- the normal map of the disparity map: per kept pixel the unit normal of the surface through its neighbours `radius` pixels away, in the
 *   CAMERA frame, in K26's layout (depth with 0 as the hole value, three fp32 planes, a uint8 image, a count), so that the maps of one frame can
 *   stand where K27 takes K26's model maps (with identity model poses: frame-to-frame tracking without a volume) and can fill the normals of
 *   K15's and K20's PLY files.  No counterpart in the reference: the semantics are defined here and pinned by the numpy oracle of
 *   tests/normals_oracle.py.  Still S2M2_ABI_VERSION 800: the entry point is added, nothing changes in place.
 *   `cloud` holds the INPUT fields of s2m2_cloud with the meaning they have in s2m2_tsdf_track_desc: the B padded maps, H, W, Hp, Wp (fused
 *   crop), camera and filter parameters, unfiltered.  Its outputs are IGNORED and the image is not needed.
 *   All in fp32, every operation ONE IEEE rounding, nothing fused into a multiply-add; division and sqrtf are correctly rounded.
 *   gate = (float)max_jump * (float)radius is formed once on the host as fp32; min_cos is converted to fp32 once on the host.
 *   Per pair b and pixel c = (v, u) of the UNPADDED image:
 *     point       z, keep = K15's (the same device functions), d = the map's disparity;   x = ((float)u - cx) * z / fx;   y = ((float)v - cy) * z / fy;
 *                 P = (x, y, z).  A pixel that is not kept is a hole.
 *     neighbours  horizontal: plus = (v, u + radius), minus = (v, u - radius);   vertical: plus = (v + radius, u), minus = (v - radius, u).
 *                 A neighbour q is USABLE iff it lies inside the H x W image, keep(q), and fabsf(d_q - d_c) <= gate (one exact subtraction; a NaN
 *                 fails).  Padded map pixels outside the crop are outside the image, whatever memory holds there.
 *     differences per pair: a = usable(plus) ? P_plus : P_c;   b = usable(minus) ? P_minus : P_c;   the pixel is a hole unless at least one of the
 *                 two is usable;   difference = a - b per component (central, forward or backward).  This gives dx (horizontal), dy (vertical).
 *     normal      n = dy x dx:   nx = dy.y*dx.z - dy.z*dx.y;   ny = dy.z*dx.x - dy.x*dx.z;   nz = dy.x*dx.y - dy.y*dx.x   (two products and one
 *                 subtraction each);   s = (nx*nx + ny*ny) + nz*nz;   a hole unless s > 0 and s is finite;   q = sqrtf(s);   n = (nx/q, ny/q, nz/q).
 *                 With x right, y down, z forward this points TOWARDS the camera: the side K24's and K26's gradients point to.
 *     view gate   m = sqrtf((x*x + y*y) + z*z);   cosv = -(((nx*x + ny*y) + nz*z) / m);   a hole unless cosv >= min_cos (a NaN fails).
 *   outputs, each optional (NULL), at least one; every pixel of every requested output is written:
 *     depth    (B,1,H,W) fp32: keep ? z : 0 -- K15's bytes, whether or not the pixel has a normal
 *     normals  (B,3,H,W) fp32: n, 0,0,0 at a hole
 *     image    (B,3,H,W) uint8: per channel (int)rintf(n_a * 127.5f + 127.5f) (one product, one sum, half to even), 0,0,0 at a hole
 *     count    (B) int32 pixels that have a normal: cleared on the stream by the entry point, then one atomic integer add per block.  The sum
 *              does not depend on the order, so the stage stays bit-reproducible.
 *   One launch plus the clear of count, no workspace, no host step.
 *   Errors (before any device call): null descriptor; everything s2m2_tsdf_track checks of its maps and camera; no output requested; depth,
 *   normals or count not 4-byte aligned; radius outside 1 .. 8; max_jump negative or NaN (+inf is allowed: it joins everything); min_cos not
 *   finite or >= 1.
 *   Non-finite maps never form an address: every index comes from integers.
 *   Launch plans: s2m2_normals is NOT recorded.  Called while the calling thread records a plan it fails with an error and launches nothing.
 *   Safe under stream capture (hipGraph).
 */
typedef struct s2m2_normals_desc {
    s2m2_cloud_desc cloud;   /* the maps: K27's meaning; outputs ignored, image not needed */
    float*   depth;          /* (B,1,H,W) fp32: K15's depth (z where keep, else 0); optional */
    float*   normals;        /* (B,3,H,W) fp32: unit normal in the CAMERA frame, towards the camera; 0,0,0 at holes; optional */
    uint8_t* image;          /* (B,3,H,W) uint8: the normal as a colour; 0,0,0 at holes; optional */
    int32_t* count;          /* (B) pixels that have a normal; optional */
    int      radius;         /* 1 .. 8: the neighbours lie `radius` pixels away */
    double   max_jump;       /* px of disparity per pixel of distance, >= 0, +inf allowed (K20's gate) */
    double   min_cos;        /* finite, < 1: smallest cosine between the normal and the direction to the camera */
} s2m2_normals_desc;
int s2m2_normals(const s2m2_normals_desc* desc, void* stream);

/*
 * K29 -- edge-preserving smoothing of the disparity map: a bilateral filter over the (2 radius + 1)^2 window of every kept pixel, in front of
 *   K15 / K20 .. K28, which all take the map exactly as it leaves the forward.  Its output has the form K22 established: a PADDED disparity map
 *   with -1 at dropped pixels, fed to any stage behind it with unfiltered = 1.  No counterpart in the reference: the semantics are defined here
 *   and pinned by the numpy oracle of tests/smooth_oracle.py.  Still S2M2_ABI_VERSION 800: two entry points are added, nothing changes in place.
 *   `cloud` holds the INPUT fields of s2m2_cloud with the meaning they have in s2m2_normals_desc: the B padded maps, H, W, Hp, Wp (fused crop),
 *   camera and filter parameters, unfiltered.  Its outputs are IGNORED and the image is not needed.
 *   The weights.  No exponential is evaluated on the device.  The host forms two tables in double and rounds each entry ONCE to fp32:
 *     ws[k] = exp(-(k*k) / (2 sigma_s^2))                                       k = 0 .. radius   (entries behind radius are 0 and never read)
 *     wr[i] = exp(-(e_i*e_i) / (2 sigma_r^2)),   e_i = i * (4 sigma_r / 256)    i = 0 .. 256
 *     inv   = (float)(256 / (4 sigma_r))
 *   s2m2_smooth_weights returns exactly the values a call of s2m2_smooth with these parameters uses; it touches no device.  The tables reach
 *   the kernel as kernel arguments: no allocation, no workspace.  gate = (float)max_jump is formed once on the host.
 *   All in fp32, every operation ONE IEEE rounding, nothing fused into a multiply-add; the division is correctly rounded.
 *   Per pair b and pixel c = (v, u) of the UNPADDED image, keep = K15's (the same device functions), d = the map's disparity:
 *     not keep(c): disp_out = -1, taps = 0.
 *     num = 0;  den = 0;  n = 0
 *     for dv = -radius .. radius:                   raster order of the window: dv outer, du inner, both ascending
 *       for du = -radius .. radius:
 *         q = (v + dv, u + du);  skipped unless q lies inside the H x W image and keep(q)
 *         e = d_q - d_c;   a = fabsf(e);   skipped unless a <= gate                                  (a NaN fails)
 *         t = fminf(a * inv, 256.f);   i = (int)t                                                   (truncation; t is in [0, 256])
 *         w = (ws[|dv|] * ws[|du|]) * wr[i]                                                         (two products)
 *         num = num + w * e;   den = den + w;   n += 1
 *     disp_out = d_c + num / den;   taps = n
 *   The centre always enters with w = 1 exactly (ws[0] = wr[0] = 1), so den >= 1.  (Two corners that only unusual parameters reach: a kept
 *   d_c = -inf -- K15 keeps d <= 0 when depth_trunc admits 1e9 / depth_scale -- fails its own gate and gives a NaN; a sigma_r so small that inv
 *   is +inf sends every tap to wr[256].)  Padded map pixels outside the crop are outside the image, whatever memory holds there.  max_jump is
 *   NOT scaled by the radius, unlike K28's: it is the largest disparity difference between the centre and a neighbour anywhere in the window.
 *   The order of the additions is part of the rule: the sum of a pixel is sequential.
 *   Non-finite maps never form an address: the only index formed from a float is i, which is clamped first (fminf returns the number when one
 *   operand is a NaN).
 *   outputs, each optional (NULL), at least one; every element of every requested output is written:
 *     disp_out (B,1,Hp,Wp) fp32, the PADDED map: the smoothed disparity where the pixel is kept, -1 everywhere else, the padding border
 *              included (K22's disp_out convention).  It must not overlap an input map: blocks read each other's halo.
 *     taps     (B,1,H,W) int32: n, the neighbours that entered the sum, the pixel itself included; 0 where the pixel is not kept
 *     count    (B) int32 kept pixels: cleared on the stream by the entry point, then one atomic integer add per block.  The sum does not
 *              depend on the order, so the stage stays bit-reproducible.
 *   One launch plus the clear of count, no workspace, no host step.
 *   Errors (before any device call): null descriptor; everything s2m2_normals checks of its maps and camera; no output requested; disp_out,
 *   taps or count not 4-byte aligned; disp_out overlapping an input map; radius outside 1 .. 8; sigma_s or sigma_r not finite or <= 0;
 *   max_jump negative or NaN (+inf is allowed: only keep decides).  s2m2_smooth_weights: a null pointer, or a bad radius or sigma.
 *   Launch plans: s2m2_smooth is NOT recorded.  Called while the calling thread records a plan it fails with an error and launches nothing.
 *   Safe under stream capture (hipGraph).
 */
typedef struct s2m2_smooth_desc {
    s2m2_cloud_desc cloud;   /* the maps: K28's meaning; outputs ignored, image not needed */
    float*   disp_out;       /* (B,1,Hp,Wp) fp32: the smoothed PADDED map, -1 where not kept and on the border; optional */
    int32_t* taps;           /* (B,1,H,W) int32: neighbours in the pixel's sum, itself included; 0 where not kept; optional */
    int32_t* count;          /* (B) kept pixels; optional */
    int      radius;         /* 1 .. 8: the window is (2 radius + 1)^2 */
    double   sigma_s;        /* pixels, finite, > 0 */
    double   sigma_r;        /* px of disparity, finite, > 0 */
    double   max_jump;       /* px of disparity, >= 0, +inf allowed; NOT scaled by the radius */
} s2m2_smooth_desc;
int s2m2_smooth(const s2m2_smooth_desc* desc, void* stream);
/* ws9: 9 floats, wr257: 257 floats, inv: 1 float; host memory.  No device is touched. */
int s2m2_smooth_weights(int radius, double sigma_s, double sigma_r, float* ws9, float* wr257, float* inv);

#ifdef __cplusplus
}
#endif
#endif /* S2M2_HIP_H */
