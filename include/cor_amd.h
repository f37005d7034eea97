/* cor_amd.h — C ABI of libcor_amd.so: the MI355X (gfx950) kernels behind the CORE retrieval-time forward path.
 *
 * The reference (wangtong627/COR) is 100 % Python and has no FFI layer: its "plugin boundary" for this path is
 * the nn.Module API (lib/build_model.py:14-20 factory, lib/sam_with_sup_branch.py:57-104 forward). The Python
 * mirror of that API lives in cor_amd/lib/; every piece of arithmetic it needs is one of the entry points below,
 * each replacing the torch op sequence cited as "ref:". A reference maintainer binds them with ctypes
 * (see INTEGRATION.md).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless the name ends in _host; no allocation happens inside;
 *  - `stream` is a hipStream_t passed as void*; kernels are only enqueued, never synchronised;
 *  - return 0 on success, a positive hipError_t for a launch failure, COR_EINVAL (-1) for bad arguments,
 *    COR_ENOSUPPORT (-2) for a shape/dtype combination that has no kernel (never a silent fallback);
 *  - activations are token-major row matrices [rows, C] (channels-last); dtypes are COR_F32 or COR_BF16 (COR_BF16X3 split rows
 *    where stated: the exact-query mode's support branch);
 *    parameters that stay in fp32 (bias, LayerNorm affine, rel-pos tables) are `const float*`.
 */
#ifndef COR_AMD_H
#define COR_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define COR_EINVAL (-1)
#define COR_ENOSUPPORT (-2)
/* Work order, OR-ed into cor_gemm's `cfg`, cor_layernorm's `act` and cor_sam_attention's `variant` (results are identical):
 * walk the output tiles / rows / windows from the LAST to the first. A kernel chain over activations larger than the 256 MB
 * Infinity Cache runs faster when each kernel starts where its producer finished (the producer's last ~200 MB are still cached):
 * the engine alternates the direction along the encoder's chain (measured +2-3 % end to end on SAM-B at batch 32). */
#define COR_ORDER_REVERSE (1 << 30)
#define COR_TOPK_FORCE_LISTS 1 /* cor_similarity_topk flags: per-lane sorted-list kernels only (no threshold-and-append) */
#define COR_TOPK_NO_FALLBACK 2  /* ... : no device-side fallback after a candidate overflow: such queries return index -2 */
#define COR_TOPK_FORCE_GLOBAL_THRESHOLD 8 /* ... : never the two-launch local-threshold path of small shards (A/B partner, tests) */
#define COR_TOPK_WAVE_FINAL 16 /* ... : global-threshold pipeline with the one-wave-per-query selection kernel fed from the records (slower A/B partner, tests) */
#define COR_TOPK_KMAX 256     /* largest k cor_similarity_topk accepts (k > 32: the wide route, see below) */
#define COR_MERGE_NMAX 4096   /* most entries per query (P * kin) one cor_merge_topk launch ranks */
#define COR_FILTER_EQ 0       /* cor_similarity_topk_filtered: a row is allowed if its label equals the query's */
#define COR_FILTER_NE 1       /* ... : a row is allowed if its label differs from the query's */

enum { COR_F32 = 0, COR_BF16 = 1, COR_F16 = 2 /* gallery storage only */, COR_BF16X3 = 3 /* x3 split rows, see below */,
       COR_I8 = 4 /* int8 rows with one fp32 scale per row; accepted only where stated */ };
/* COR_BF16X3 (exact-query mode: the support branch at fp32 accuracy on the bf16 matrix cores). An fp32 value x is carried as
 * hi = bf16_rne(x) and lo = bf16_rne(x - hi); a SPLIT ROW of C logical values is bf16 [lo(0..C) | hi(0..C) | hi(0..C)] (3C elements,
 * segment stride C unless stated), a split WEIGHT row is [hi | lo | hi]. A bf16 GEMM over the 3K columns then computes
 * A_lo.W_hi + A_hi.W_lo + A_hi.W_hi into ONE fp32 accumulator in that order (error ~1e-6 of sum|a.b| at K = 768, ~500x below bf16).
 * Accepted as cor_gemm's ab_dtype, cor_layernorm's y_dtype (fp32 x), cor_attention_f32's out_dtype; cor_split_x3 makes it from fp32. */
enum { COR_ACT_NONE = 0, COR_ACT_GELU_ERF = 1, COR_ACT_RELU = 2, COR_ACT_SIGMOID = 3, COR_ACT_GELU_TANH = 4 };

int cor_version(void);

/* ---- dense linear algebra -------------------------------------------------------------------------------- */

/* C[M,N] = residual + col_scale * act(A[M,K] . W[N,K]^T + bias)          (nn.Linear / 1x1 conv / patch conv)
 * A, W share `ab_dtype`; bias/col_scale [N] fp32 or NULL; residual fp32 [*, ldr] or NULL, read at row
 * (m % res_row_mod) when res_row_mod > 0 (broadcast of pos_embed over the batch).
 * MFMA path: v_mfma_f32_32x32x16_bf16 (bf16) or v_mfma_f32_32x32x2_f32 (exact fp32).
 * ref: every nn.Linear on the path, e.g. lib/sam_model/image_encoder.py:229,239 ; common.py:25-26 ;
 *      PatchEmbed conv image_encoder.py:386-394 (as GEMM over patches) ; neck 1x1 conv :87-92. */
int cor_gemm(const void* A, long lda, const void* W, long ldw, int ab_dtype,
             void* C, long ldc, int c_dtype, int M, int N, int K,
             const float* bias, int act, const float* col_scale,
             const float* residual, long ldr, int res_row_mod, int cfg, void* stream);
/* ab_dtype COR_BF16X3: A [M, >= 3K] split rows, W [N, >= 3K] split weight rows, K the LOGICAL depth; c_dtype COR_F32 or COR_BF16.
 * Every cfg (and COR_ORDER_REVERSE) applies unchanged: the kernels run their K loop over the three K segments.
 * ref: the support branch's nn.Linear / 1x1 convs in exact-query mode (lib/support_branch.py:56-87, siglip_openclip.py:30-59). */
/* `cfg` is a PER-CALL kernel choice (no process-global state; safe from several threads / streams): 0 = automatic
 * (13 for bf16 operands from 200 output tiles of 256x256 up, else 2, or 1 when K has a ragged tail); 1: 128x128 register-staged
 * (any K); 2: 128x128 LDS-DMA; 3 / 4: 128x64 / 64x64; 9: 256x128, three LDS buffers; 13: persistent 256x256 ping-pong kernel
 * (bf16 operands; falls back to 2 / 1 where it does not apply); optionally | COR_ORDER_REVERSE. Anything else is COR_EINVAL:
 * the timing probes of the development builds (result-destroying ablation bits, 16x16 MFMA form) are not in this library
 * (they build into tools/probes/libcor_probes.so with -DCOR_PROBES). */

/* What cor_gemm would run for these arguments (cor_gemm's, without `stream`; pointer VALUES matter: alignment selects the scalar kernel
 * and the scalar epilogue). Pure host function, no launch. Returns the kernel - 1, 2, 3, 4, 9 or 13 as in `cfg`, after every demotion
 * (2 / 3 / 4 / 9 -> 1 on a ragged K tail, 13 -> 2 / 1 where the persistent kernel does not apply), or COR_GEMM_KERNEL_SCALAR for the
 * scalar kernel of unaligned operands - OR-ed with COR_GEMM_EPILOGUE_VEC when the tile kernel takes its 16-byte vector epilogue
 * (else the per-element one); or the COR_EINVAL / COR_ENOSUPPORT cor_gemm would return. */
#define COR_GEMM_KERNEL_SCALAR 32
#define COR_GEMM_KERNEL_MASK 0xff
#define COR_GEMM_EPILOGUE_VEC (1 << 8)
int cor_gemm_kernel_id(const void* A, long lda, const void* W, long ldw, int ab_dtype,
                       const void* C, long ldc, int c_dtype, int M, int N, int K,
                       const float* bias, int act, const float* col_scale,
                       const float* residual, long ldr, int res_row_mod, int cfg);

/* y[r,:] = LayerNorm(x[r,:]) * w + b over the last dim, biased variance.
 * ref: nn.LayerNorm (image_encoder.py:169,183), LayerNorm2d common.py:31-43 and mask_adapter.py:226-251 (on
 *      channels-last rows), transformer.py norm1..4. */
int cor_layernorm(const void* x, int x_dtype, void* y, int y_dtype, const float* w, const float* b,
                  int rows, int C, float eps, int act, void* stream);
/* y_dtype COR_BF16X3 (x fp32): y [rows, 3C] split rows, the A operand of the next x3 GEMM (SigLIP norm1 / norm2 / ln_1 / ln_2 ->
 * qkv / fc1 in exact-query mode: timm vision_transformer Block, open_clip ResidualAttentionBlock). */

/* ---- attention -------------------------------------------------------------------------------------------- */

/* out[b,t,h,:] = softmax_k(scale * q[b,t,h,:].k[b,k,h,:]) v ; element (b,t,h,c) of X lives at
 * X + b*x_sb + t*x_st + h*hd + c (strides in elements). hd in {16,32,64,72,80}; bf16 with hd 64 / 72 / 80 and >= 64 queries and
 * keys runs the MFMA flash kernel (72 = SigLIP SO400M/14, the factory's default tower), everything else the row-per-lane kernel.
 * ref: lib/sam_model/transformer.py:218-240 (decoder Attention), SigLIP towers' MHA.
 * PRECONDITION (cor_attention and cor_sam_attention, bf16 MFMA kernels): q, k, v are FINITE. The softmax of those kernels is compiled
 * with -fno-honor-nans (no NaN arises inside: the running maximum starts at -inf, every key tile holds a real key; -inf marks padded
 * key slots and is honoured), so a NaN / Inf operand from upstream (e.g. a bf16 overflow) gives unspecified values in the rows of the
 * (sample, head) that contain it instead of a propagated NaN; other (sample, head) pairs are unaffected (tests/test_gpu_parity.py::
 * test_attention_nonfinite_operands_stay_inside_their_head). The fp32 row-per-lane kernels propagate NaN as IEEE arithmetic does. */
int cor_attention(const void* q, long q_sb, long q_st, const void* k, long k_sb, long k_st,
                  const void* v, long v_sb, long v_st, int dtype,
                  void* out, long o_sb, long o_st, int out_dtype,
                  int B, int H, int Tq, int Tk, int hd, float scale, void* stream);

/* flash_fwd_f32: the same plain MHA as cor_attention with fp32 q / k / v, on the f32-input matrix cores (v_mfma_f32_16x16x4_f32: exact
 * f32 products, fp32 online softmax, P kept in fp32): the SigLIP towers of exact-query mode. hd in {64, 72, 80}, any Tq / Tk >= 1;
 * k / v 16-byte aligned, all strides multiples of 4. out_dtype COR_F32 (out [.., H*hd] rows) or COR_BF16X3 (split rows of H*hd logical
 * values: o_st >= 3*H*hd bf16 elements), i.e. the A operand of the proj GEMM. cor_attention's fp32 path (row-per-lane kernel) is unchanged.
 * ref: SigLIP towers' MHA (timm Attention, open_clip nn.MultiheadAttention; siglip_openclip.py:30-59). */
int cor_attention_f32(const float* q, long q_sb, long q_st, const float* k, long k_sb, long k_st,
                      const float* v, long v_sb, long v_st, void* out, long o_sb, long o_st, int out_dtype,
                      int B, int H, int Tq, int Tk, int hd, float scale, void* stream);

/* SAM ViTDet attention on the fused qkv activation [B*grid*grid, 3*H*hd] (q|k|v, head-major inside each;
 * hd = 64 for SAM-B/L and 80 for SAM-H (bf16: MFMA flash kernels), 16/32 for reduced test models (row-per-lane kernel)):
 * logits = (q*hd^-0.5).k + q.Rh[qh-kh+S-1] + q.Rw[qw-kw+S-1] (rel-pos from the UNSCALED q).
 * window == 0: global attention over the grid (S = grid). window > 0: non-overlapping window x window tiles of the
 * grid zero-padded bottom/right to a multiple of `window` AFTER norm1, so a padded token's q/k/v equal the qkv
 * bias (`pad_row`, [3*H*hd] in `dtype`); padding/partition/unpartition are folded into addressing.
 * out [B*grid*grid, H*hd]. rel_h / rel_w: [2S-1, hd] fp32.
 * ref: lib/sam_model/image_encoder.py:225-241 (Attention), :244-290 (window partition), :293-362 (rel-pos). */
int cor_sam_attention(const void* qkv, int dtype, void* out, int out_dtype, const void* pad_row,
                      const float* rel_h, const float* rel_w, int B, int H, int hd, int grid, int window, float q_prescale, int variant,
                      void* stream);
/* `q_prescale`: the factor the caller has ALREADY folded into the q third of qkv (and of pad_row): 1 = raw q (always accepted);
 * 0.125 * log2(e) (hd 64: scale * log2 e) lets the bf16 MFMA kernels run the score product directly in the log2 domain with
 * no per-score multiply - the engine folds it into the q rows of the qkv weight / bias at pack time, so it costs nothing at
 * run time and q is rounded to bf16 once. The rel-pos terms are rescaled accordingly inside (they use the unscaled q).
 * `variant` is a PER-CALL kernel choice for the bf16 MFMA path: 0 = default kernels (global: flash_global_pipe, software-
 * pipelined over key tiles, with a pre-scaled q the column bias is the score MFMA's start value; windowed: win_attn, one 7-wave
 * block per (window, head)); 1 = the round-1 chain forms of the same arithmetic (flash_fwd<1> / flash_fwd<2>), kept as the
 * in-process A/B and parity partners (tests, tools/attn_bench.py); 2 = flash_global_pipe with the bias as one fma per score
 * (round 4's default; A/B partner); 4 = flash_global_w64 (global, pre-scaled q only: 64 queries per wave at one wave per SIMD;
 * parity-tested, measured slower: DESIGN 3.2); 2 and 4 select the default kernel where they do not apply (windowed, raw q);
 * optionally | COR_ORDER_REVERSE. Anything else is COR_EINVAL (the timing probe of the global kernel, which writes cycle
 * counters instead of outputs, exists in -DCOR_PROBES builds only: tools/probes/libcor_probes.so, tools/attn_stamps.py). */

/* Which kernel family cor_attention (sam_window = -1) / cor_sam_attention (0 = global, > 0 = windowed) runs for 16-byte-aligned
 * operands of this shape: bf16 with head_dim 64 / 72 / 80 is on the matrix cores. Pure function (no launch). */
enum { COR_KERNEL_ROWLANE = 1, COR_KERNEL_FEWQ = 2, COR_KERNEL_FLASH_MFMA = 3, COR_KERNEL_FLASH_PIPELINED = 4, COR_KERNEL_WINDOW_BLOCK = 5 };
int cor_attention_kernel_id(int dtype, int hd, int Tq, int Tk, int sam_window, int grid);

/* ---- data movement / elementwise --------------------------------------------------------------------------- */

/* Non-overlapping p x p patches of NCHW fp32 images -> rows [B*(H/p)*(W/p), Kpad] (k = c*p*p + dy*p + dx, zero
 * padded to Kpad), i.e. the A operand of the patch-embedding GEMM; floor division: a ragged right/bottom border is
 * dropped as a strided conv does (SO400M/14 at 384 px: 27x27 patches). ref: image_encoder.py:386-394. */
int cor_patchify(const float* img, void* out, int out_dtype, int B, int C, int H, int W, int p, int Kpad, void* stream);

/* 3x3, pad 1 im2col of channels-last tokens [B,H,W,C] -> [B*H*W, 9*C] (k = (ky*3+kx)*C + c).
 * ref: neck conv image_encoder.py:94-100. */
int cor_im2col3x3(const void* x, int dtype, void* out, int B, int H, int W, int C, void* stream);

/* out = a + b[(i) % b_period] elementwise over n elements (b_period = n for a plain add). */
int cor_add(const void* a, int a_dtype, const void* b, int b_dtype, void* out, int out_dtype, long n, long b_period, void* stream);

/* dtype cast / strided row copy: out[r, :C] = in[r, :C]; ld_in == 0 broadcasts one source row. */
int cor_copy_rows(const void* in, long ld_in, int in_dtype, void* out, long ld_out, int out_dtype, int rows, int C, void* stream);

/* fp32 -> split rows (COR_BF16X3): out[r*ld_out + c] = lo, out[r*ld_out + seg + c] = out[r*ld_out + 2*seg + c] = hi for c < C
 * (seg >= C: several logical column blocks can share one split row, e.g. [image | text] of the fusion gates; ld_out >= 2*seg + C).
 * ref: the casts ahead of the support branch's GEMMs in exact-query mode (mask_adapter.py:90,163, cir_feature_fuse.py:44-58,
 *      support_branch.py:86, patch embedding). */
int cor_split_x3(const float* in, long ld_in, void* out, long ld_out, long seg, int rows, int C, void* stream);

/* [rows, C] channels-last tokens -> NCHW [B, C, HW] (fp32 out) and back. */
int cor_tokens_to_nchw(const void* x, int dtype, float* out, int B, int HW, int C, void* stream);
int cor_nchw_to_tokens(const float* x, void* out, int out_dtype, int B, int HW, int C, void* stream);

/* y = x / max(||x||_2, eps) per row. ref: F.normalize (support_branch.py:85, cir_feature_fuse.py:58, siglip_openclip.py:56). */
int cor_l2norm_rows(const void* x, int x_dtype, void* y, int y_dtype, int rows, int C, float eps, void* stream);

/* out[r,:] = table[ids[r],:] + pos[r % ctx,:]. An id outside [0, vocab) (nn.Embedding raises; a wrong tokenizer) makes the
 * row NaN: never a fault, never plausible garbage. ref: open_clip TextTransformer embedding (siglip_openclip.py:53). */
int cor_embed_tokens(const long long* ids, const float* table, const float* pos, float* out, int rows, int ctx, int D, int vocab, void* stream);

/* ---- support branch (mask adapter, fusion) ------------------------------------------------------------------ */

/* Bilinear resize, align_corners=False, no antialias, fp32 NCHW planes. ref: F.interpolate at mask_adapter.py:20,58,158. */
int cor_bilinear(const float* x, float* out, int planes, int H, int W, int OH, int OW, int clamp01, void* stream);

/* Direct 3x3 stride-2 pad-1 convolution for tiny channel counts, NCHW fp32 in, channels-last fp32 out
 * [B, OH, OW, Cout]. ref: mask_adapter.py:128-137 (mask_downscaling convs). */
int cor_conv3x3s2_small(const float* x, int x_channels_last, const float* w, const float* bias, float* out,
                        int B, int Cin, int Cout, int H, int W, void* stream);

/* Depthwise 7x7 pad 3 on channels-last tokens [B,H,W,C] fp32 -> out (dtype). w_t [49,C] (tap-major transpose of
 * the reference's [C,1,7,7] weight, made once at load), bias [C]. ref: mask_adapter.py:197-199 (ConvNextBlock.dwconv). */
int cor_dwconv7x7(const float* x, const float* w_t, const float* bias, void* out, int out_dtype, int B, int H, int W, int C, void* stream);

/* pooled[b,:] = mean_m sum_p softmax_p(logsigmoid(maps[b,p,m])) feat[b,p,:]   (maps [B,P,M] fp32, feat [B,P,D] fp32)
 * ref: mask_adapter.py:68-79. */
int cor_adapter_pool(const float* maps, const float* feat, float* out, int B, int P, int M, int D, void* stream);

/* pooled[b,:] = sum_p feat[b,p,:]*mask[b,p] / (sum_p mask[b,p] + 1e-8), optional clamp of mask to [0,1] and
 * L2-normalisation. ref: mask_adapter.py:13-25 (MaskedPooling), utils/loss_func.py:35-56 (region embedding;
 * feat there is NCHW: pass feat_nchw=1). */
int cor_masked_pool(const float* feat, int feat_nchw, const float* mask, float* out, int B, int P, int D,
                    int clamp01, int l2norm, void* stream);

/* Region pooling for a multi-region gallery: R masks pooled against the tokens of B images, every image's tokens read once per
 * tile of 8 regions instead of once per region. tokens f32 [B,P,D] channels-last (the SAM encoder's output: P = grid^2, D = 256);
 * masks f32 [R,P], one plane per region at grid resolution; region_offsets int32 [B+1] in DEVICE memory, CSR layout: regions
 * [off[b], off[b+1]) belong to image b (non-decreasing, off[0] = 0, off[B] = R; an image may have none). out [R,D] in out_dtype
 * (COR_F32, COR_BF16 or COR_F16; 16-bit outputs are the f32 result rounded to nearest-even).
 *   out[r,:] = sum_p tokens[b,p,:]*m[r,p] / (sum_p m[r,p] + 1e-8), m clamped to [0,1] if clamp01, L2-normalised if l2norm
 * with the summation orders of cor_masked_pool: a COR_F32 row is bit-identical to cor_masked_pool(tokens + b*P*D, 0, masks + r*P,
 * B = 1, ...), so a gallery row does not depend on how many regions share its image, on their order or on the tiling.
 * The host cannot see the offsets: the kernel clamps them into [0, R] and never reads or writes outside the three arrays (rows that
 * inconsistent offsets leave uncovered are not written). R == 0 or B == 0: returns 0 without a launch. D <= 1024 (the tile's pooled
 * rows wait in LDS for the norm), larger: COR_ENOSUPPORT; a bad out_dtype: COR_EINVAL.
 * ref: utils/loss_func.py:35-56 (region embedding) applied to every region of an image. */
int cor_region_pool(const float* tokens, const float* masks, const int* region_offsets, void* out, int out_dtype, int B, int R,
                    int P, int D, int clamp01, int l2norm, void* stream);

/* i' = aI*i ; t' = aT*t  (gates already sigmoid-ed), written into cat [N,2D]; and the final
 * out = normalize(dyn*i' + (1-dyn)*t'). ref: cir_feature_fuse.py:51-58. */
int cor_fuse_gate(const float* img, const float* txt, const float* aI, const float* aT, float* cat, int N, int D, void* stream);
int cor_fuse_mix(const float* cat, const float* dyn, float* out, int N, int D, void* stream);

/* ---- prompt encoder / mask decoder ------------------------------------------------------------------------- */

/* Random-Fourier dense PE as tokens [size*size, 2F] fp32: cat(sin,cos)(2*pi*((2*xy-1) @ G)), G [2,F].
 * ref: my_prompt_encoder.py:62-71,191-211. */
int cor_dense_pe(const float* gauss, float* out, int size, int F, void* stream);

/* Pixel-shuffle of a ConvTranspose2d(k=2,s=2) computed as GEMM: y[B*H*W, 4*Cout] (col = (dy*2+dx)*Cout + co, the
 * order the weight is packed in at load) -> out[B, 2H, 2W, Cout] (+ bias), then optional LayerNorm over Cout
 * (ln_w/ln_b both NULL to skip) and activation.
 * ref: mask_decoder.py:54-60 (output_upscaling). */
int cor_upscale_shuffle(const void* y, int y_dtype, const float* bias, const float* ln_w, const float* ln_b, float eps,
                        int act, void* out, int out_dtype, int B, int H, int W, int Cout, void* stream);

/* Fused second upscaling + hypernetwork product:
 * masks[b,k,2y+dy,2x+dx] = sum_co hyper[b,k,co] * gelu( sum_ci x[b,y,x,ci] * w[ci,co,dy,dx] + bias[co] )
 * x [B,H,W,Cin] (dtype), w [Cin,Cout,2,2] fp32, hyper [B,Kmask,Cout] fp32 -> masks [B,Kmask,2H,2W] fp32.
 * ref: mask_decoder.py:58-59,133-137. */
int cor_upscale_hyper(const void* x, int dtype, const float* w, const float* bias, const float* hyper, long hyper_bs,
                      float* masks, int B, int H, int W, int Cin, int Cout, int Kmask, void* stream);

/* best[b] = argmax_k iou[b, k_off : k_off+Ksel] (first maximum wins, like torch.argmax);
 * hyper_sel[b,:] = hyper[b, k_off+best[b], :]  ([B,Kall,C] -> [B,C]). Selecting the hypernetwork row BEFORE the
 * upscaling means only the chosen mask channel is ever computed / written.
 * ref: sam_with_sup_branch.py:96-100 ; mask_decoder.py:97-102. */
int cor_iou_select(const float* iou, const float* hyper, int B, int Kall, int k_off, int Ksel, int C, long long* best,
                   float* hyper_sel, void* stream);

/* The decoder's five output MLPs in one launch: hyper-network MLP i (i = 0..3) on mask token 1+i -> hyper[b, i, 0:32], IoU head on token 0
 * -> iou[b, 0:4]; each Linear(256,256) ReLU Linear(256,256) ReLU Linear(256, 32 | 4). hs [B,6,256] in `dtype` (COR_F32 | COR_BF16, the
 * weights' type too); w01 [5,2,256,256] (MLP, layer, out, in; MLP 4 = IoU head), b01 [5,2,256] fp32, w2 [132,256] (rows 32 i + c of
 * hyper MLP i, rows 128..131 of the IoU head), b2 [132] fp32. fp32 accumulation over k in order; hidden activations rounded to `dtype`.
 * ref: mask_decoder.py:123-140 (output_hypernetworks_mlps, iou_prediction_head), :147-167 (MLP). */
int cor_decoder_heads(const void* hs, const void* w01, const float* b01, const void* w2, const float* b2, int dtype, float* hyper,
                      float* iou, int B, void* stream);

/* ---- inference harness (mask post-processing, metrics) ---------------------------------------------------------------- */

/* out = (sigmoid(x) - min) / (max - min + 1e-8), min/max per sample. ref: utils/vailder.py:426-430. */
int cor_mask_prob_minmax(const float* logits, float* out, int B, int HW, void* stream);

/* Bilinear resize (half-pixel centres, edge clamp = cv2.INTER_LINEAR) of [B,H,W] probabilities to [B,OH,OW], then
 * (> threshold) ? 255 : 0 as uint8. ref: utils/vailder.py:459-473. */
int cor_resize_binarize(const float* prob, unsigned char* out, int B, int H, int W, int OH, int OW, float threshold, void* stream);

/* The same resize, then (v * 255) truncated to uint8: the soft (grayscale) mask of save_soft_pred_masks.
 * ref: utils/vailder.py:513-656 (:615-621: cv2.resize INTER_LINEAR, (pred * 255).astype(np.uint8)). */
int cor_resize_gray(const float* prob, unsigned char* out, int B, int H, int W, int OH, int OW, void* stream);

/* out[b] = {dice, mae, iou, mdice, miou} of a soft prediction against the ground truth, [B,HW] each.
 * ref: utils/trainer_v3_g.py:381-443 (compute_dice / compute_mae / compute_iou / compute_mdice / compute_miou). */
int cor_mask_metrics(const float* pred, const float* gt, float* out, int B, int HW, float smooth, void* stream);

/* ---- input pre-processing (device side of utils/dataloader.py:266-293) ------------------------------------------------ */

/* Pillow-BILINEAR resize of uint8 images, as torchvision.transforms.Resize performs it on a PIL image (Pillow
 * src/libImaging/Resample.c, 8 bits per channel, antialiased on down-scaling), bit-exact. The caller supplies Pillow's
 * fixed-point tables for one axis: bounds int32[out,2] = (first input index, tap count), kk int32[out,ksize] =
 * int(0.5 + w * 2^22) (cor_amd/preprocess.py:resample_tables). Pass 1: rows. in u8[H,W,C] -> out u8[H,OW,C]; C in {1,3}. */
int cor_resample_rows_u8(const unsigned char* in, unsigned char* out, const int* bounds, const int* kk, int ksize, int H, int W, int C,
                         int OW, void* stream);

/* Pass 2: columns of the uint8 image pass 1 produced, then ToTensor (+ Normalize): in u8[H,W,C] -> out_u8 u8[OH,W,C] (may be
 * NULL) and out_f32 f32[C,OH,W] (may be NULL) = v/255, or (v/255 - mean[c]) / std[c] when mean/std are given (both or
 * neither), in IEEE float32 exactly as torchvision's ToTensor / Normalize compute it. */
int cor_resample_cols_u8(const unsigned char* in, float* out_f32, unsigned char* out_u8, const int* bounds, const int* kk, int ksize, int H,
                         int W, int C, int OH, const float* mean, const float* stdv, void* stream);

/* ---- retrieval ------------------------------------------------------------------------------------------------ */

/* Per query b: the top-k rows g of the gallery shard by score = q[b,:].G[g,:] (fp32 accumulate), ordered by
 * (score desc, index asc); indices are returned as global ids (g + g_offset).
 * Q [Bq,C] fp32, G [Ng,C] in g_dtype (COR_F32 exact chain / COR_BF16 / COR_F16), C <= 256 and C % 16 == 0, 1 <= k <= COR_TOPK_KMAX (256);
 * missing entries (Ng < k) come back as score -inf, index -1. workspace >= cor_topk_workspace_bytes(Bq,Ng,k).
 * The reference has no gallery/top-k code; the definition follows utils/loss_func.py:84 (cosine of unit vectors).
 * Scores are DEFINED as the fp32 fmaf chain of oracle/c/sim_chain.c (16-bit rows widened exactly), for every gallery dtype: the
 * result is bit-identical to that CPU chain, scores and indices. fp32 shards run the chain kernel. 16-bit shards (C = 256) scan on the
 * matrix cores and re-score a short list with the exact chain: SMALL shards (<= 32 slices of 256..1024 rows per query in one round of
 * blocks, k <= 16: the 8-GPU shard shapes, 256..512 queries x 12.5k rows) in TWO launches with block-local thresholds (sim_block_scan:
 * every block bounds its queries' k-th best score from the maxima of 32 disjoint row classes of its own slice and appends what passes;
 * sim_final_wave: one wave per query selects, re-scores, ranks); everything else by threshold-and-append with a GLOBAL threshold (a strided
 * sample pass bounds each query's k-th best score by 32 super-group maxima, the full MFMA pass ranks them in its prologue and appends the
 * rare score records above the bound, the final pass re-scores the short list: four launches). If a query's candidate list overflows (pathological score distributions, e.g. hundreds of identical rows)
 * it is ranked by an exact brute-force chain pass ON THE DEVICE (no host round trip). All of the above is k <= 32.
 * 33 <= k <= 256 (WIDE k: Recall@50/100, two-stage re-ranking) takes its own route, bit-identical to the chain oracle for EVERY g_dtype and C
 * (for 16-bit galleries with C != 256 that is stronger than k <= 32 promises): a strided sample pass keeps >= 2k group maxima per query, a
 * small kernel ranks them into the bound tau_q, the full scan appends the scores >= tau_q (16-bit C = 256: the threshold-and-append scan
 * above; fp32 and 16-bit C != 256: the tile kernels of the list path), and one block per query selects the exact k-th best scan score,
 * re-scores the short list with the chain (16-bit) and ranks it with a bitonic sort. An overflowed query is ranked in the same block by a
 * radix select over the chain scores of the whole shard (exact; tens of ms at 1M rows). Wide k: COR_TOPK_FORCE_LISTS and COR_TOPK_WAVE_FINAL
 * return COR_ENOSUPPORT, COR_TOPK_FORCE_GLOBAL_THRESHOLD has no effect, COR_TOPK_NO_FALLBACK keeps its meaning. k > 256: COR_ENOSUPPORT
 * (cor_topk_workspace_bytes: COR_EINVAL). `flags` (per call, no process-global state):
 * 0 = default; COR_TOPK_FORCE_LISTS = per-lane sorted-list kernels only; COR_TOPK_NO_FALLBACK = report an overflow as index -2 in every
 * slot of the query instead of falling back (tests); COR_TOPK_FORCE_GLOBAL_THRESHOLD / COR_TOPK_WAVE_FINAL = A/B partners (tests). */
long cor_topk_workspace_bytes(int Bq, int Ng, int k);
int cor_similarity_topk(const float* Q, const void* G, int g_dtype, int Bq, int Ng, int C, int k, long long g_offset,
                        float* out_scores, long long* out_idx, void* workspace, int flags, void* stream);

/* Filtered top-k: per query b, the top-k of the ALLOWED gallery rows only, ordered by (score desc, global index asc), indices global
 * (g + g_offset). Every row has an int32 label row_labels[g] (shard-local row g; 16-byte aligned), every query an int32 label
 * query_labels[b]. Row g is allowed for query b if query_labels[b] < 0 (unrestricted), else, by filter_mode, if
 * row_labels[g] == query_labels[b] (COR_FILTER_EQ: restrict to a class or subset) or row_labels[g] != query_labels[b] (COR_FILTER_NE:
 * exclude a source, e.g. the query's own image). Scores are the fmaf-chain scores of cor_similarity_topk: the result is bit-identical to
 * the chain oracle run on the allowed rows, scores and indices, for COR_F32 / COR_BF16 / COR_F16, every C that cor_similarity_topk
 * accepts and 1 <= k <= COR_TOPK_KMAX. A query with fewer than k allowed rows gets them first and then the (-inf, -1) tail; a query with
 * no allowed row gets only the tail. Other arguments and alignment as for cor_similarity_topk; workspace >=
 * cor_topk_filtered_workspace_bytes(Bq, Ng, k). A null label pointer or a bad filter_mode: COR_EINVAL.
 * Route: every filtered call, whatever k, takes the wide route above with the filter inside the scans: a disallowed score is -inf before
 * the sample's group values, the threshold and the append decision (which tests the allow predicate, so tau_q = -inf never admits a
 * disallowed row). The sample keeps the four best allowed scores per group and the scan slices walk the gallery interleaved, so a
 * class-sorted gallery (one label's rows in one block) neither loses its threshold nor crowds a few candidate streams. An overflowed
 * query is ranked over its allowed rows by the in-kernel brute force. Flags: COR_TOPK_NO_FALLBACK keeps its meaning (index -2 in every
 * slot of an overflowed query); COR_TOPK_FORCE_LISTS and COR_TOPK_WAVE_FINAL return COR_ENOSUPPORT; COR_TOPK_FORCE_GLOBAL_THRESHOLD has
 * no effect. */
long cor_topk_filtered_workspace_bytes(int Bq, int Ng, int k);
int cor_similarity_topk_filtered(const float* Q, const void* G, int g_dtype, int Bq, int Ng, int C, int k, long long g_offset,
                                 const int* row_labels, const int* query_labels, int filter_mode, float* out_scores, long long* out_idx,
                                 void* workspace, int flags, void* stream);

/* Threshold (range) search: per query b, the rows that score at least thresholds[b], and how many there are.
 *   score(b, g)  = the fp32 fmaf-chain score of cor_similarity_topk (oracle/c/sim_chain.c; 16-bit rows widened exactly, the query rounded
 *                  to the gallery dtype), for COR_F32 / COR_BF16 / COR_F16 and every C that call takes.
 *   In(b)        = { g < Ng : score(b, g) >= thresholds[b] } by the IEEE comparison: a NaN floor gives the empty set, -inf every row,
 *                  +0.0 and -0.0 are the same floor. thresholds: device f32 [Bq].
 *   out_count[b] = |In(b)| (device i32 [Bq]), EXACT for every Ng: COR_TOPK_KMAX caps the listed rows only.
 *   out_scores / out_idx [Bq,k], 1 <= k <= COR_TOPK_KMAX: the first k members of In(b) by (score desc, global index asc), indices
 *                  g + g_offset, then the (-inf, -1) tail: cor_similarity_topk's lists with every entry below the floor turned into tail.
 * Scores, indices and counts are bit-identical to that definition evaluated on the CPU, for every dtype, C and k.
 * Route: every call, whatever k, takes the wide route of cor_similarity_topk (sample pass, tau_q by sim_tau_wide). With delta_q the bound
 * of |scan score - chain score| that route already uses (0 for fp32 rows), the full scan sorts every scan score s into: s >= max(tau_q,
 * thr_q - delta_q): a list candidate, appended as before; s >= thr_q + delta_q: a sure member, counted in a register of its stream and
 * written once per slice (no atomics); thr_q - delta_q <= s < thr_q + delta_q: a band row, appended so that the chain decides it. delta_q
 * is twice the bound, so s >= thr_q + delta_q implies chain >= thr_q and s < thr_q - delta_q implies chain < thr_q (rows of unit norm, as
 * for the lists). The selection kernel ranks the candidates, drops ranked rows whose chain score is below the floor, re-scores the band
 * rows and adds those at or above the floor to the summed sure counts. A candidate overflow (which may have lost band rows), or more than
 * 16 384 band rows of one query, sends the query to a chain pass over the shard that ranks AND counts in the same block (exact; slow;
 * rare: ~4 ms per query at 1M rows).
 * Argument checks and codes in cor_similarity_topk's order; a null thresholds or out_count: COR_EINVAL. Flags: COR_TOPK_NO_FALLBACK keeps
 * its meaning (an overflowed query returns index -2 in every slot and count -2); every other flag: COR_ENOSUPPORT.
 * workspace >= cor_range_workspace_bytes(Bq, Ng, k) (>= cor_topk_workspace_bytes at k >= 33). No allocation, no host synchronisation;
 * capturable in a graph. */
long cor_range_workspace_bytes(int Bq, int Ng, int k);
int cor_similarity_range(const float* Q, const void* G, int g_dtype, int Bq, int Ng, int C, const float* thresholds, int k, long long g_offset,
                         float* out_scores, long long* out_idx, int* out_count, void* workspace, int flags, void* stream);

/* Filtered threshold search: cor_similarity_range over the rows a query is allowed to see.
 *   score(b, g)  = the chain score of cor_similarity_topk, as above.
 *   Allowed(b)   = the rule of cor_similarity_topk_filtered: query_labels[b] < 0 is unrestricted; COR_FILTER_EQ allows the rows whose label
 *                  equals the query's, COR_FILTER_NE the rows whose label differs (row_labels int32 [Ng], 16-byte aligned; query_labels
 *                  int32 [Bq]; both on the device).
 *   In(b)        = { g in Allowed(b) : score(b, g) >= thresholds[b] } by the IEEE comparison (NaN: the empty set; -inf: every allowed row;
 *                  +0.0 and -0.0 are one floor).
 *   out_count[b] = |In(b)|, EXACT for every Ng; out_scores / out_idx [Bq,k]: the first k members by (score desc, global index asc), then
 *                  the (-inf, -1) tail: cor_similarity_topk_filtered's lists with every entry below the floor turned into tail. A query
 *                  with no allowed row gets count 0 and only the tail.
 * Scores, indices and counts are bit-identical to that definition for COR_F32 / COR_BF16 / COR_F16 rows, every C the top-k takes and
 * 1 <= k <= COR_TOPK_KMAX.
 * Route: the filtered plan of cor_similarity_topk_filtered (interleaved slices, four sample values per group, slices of <= 128 super-tiles,
 * so tau_q is a bound over ALLOWED rows) with the range call's six extra places per stream, bounds and sure counts. The scans mask a
 * disallowed score to -inf first and sort the masked scores as cor_similarity_range does; the bounds are floored at -3e38, so a masked
 * score is never counted, never a band row and never appended. The selection is the range call's; its fallback (candidate overflow, or
 * more than 16 384 band rows) counts and ranks the allowed rows only, over the chain. The 16-bit scan (C = 256) runs with query groups of
 * 256 (QB = 1) for every Bq: the 512-query form cannot hold labels and range state in registers together (it spilled), so a batch of more
 * than 256 queries streams the gallery once per 256 queries.
 * Argument checks before any HIP call, in cor_similarity_range's order and with its codes; the label checks are those of
 * cor_similarity_topk_filtered (a null label pointer, a bad filter_mode, row_labels not 16-byte aligned: COR_EINVAL). Flags:
 * COR_TOPK_NO_FALLBACK keeps its meaning (index -2 in every slot and count -2); every other flag: COR_ENOSUPPORT.
 * workspace >= cor_range_filtered_workspace_bytes(Bq, Ng, k) (positive for Ng up to 2^31 - 1; >= cor_topk_filtered_workspace_bytes at the
 * same arguments). No allocation, no host synchronisation; capturable in a graph. */
long cor_range_filtered_workspace_bytes(int Bq, int Ng, int k);
int cor_similarity_range_filtered(const float* Q, const void* G, int g_dtype, int Bq, int Ng, int C, const float* thresholds, int k,
                                  long long g_offset, const int* row_labels, const int* query_labels, int filter_mode, float* out_scores,
                                  long long* out_idx, int* out_count, void* workspace, int flags, void* stream);

/* Distinct-group top-k: every gallery row g has an int32 group id row_groups[g] (shard-local row g; 16-byte aligned; typically the source
 * image of a region); a negative id makes the row a group of its own. Per query b, among the rows ALLOWED for b, each group's
 * representative is its best row by (chain score desc, global index asc), and the result is the k best representatives ordered the same
 * way: out_scores f32[Bq,k], out_idx i64[Bq,k] = the representative ROWS as global ids (g + g_offset), so no group appears twice. Fewer
 * than k groups with an allowed row: those first, then the (-inf, -1) tail. Allowed = every row when row_labels and query_labels are both
 * NULL, else the rows the filter of cor_similarity_topk_filtered allows (row_labels / query_labels / filter_mode as there; filter labels
 * and group ids are separate vectors and may be the same memory). Scores are the fmaf-chain scores of cor_similarity_topk: the result is
 * bit-identical to "chain-rank the allowed rows, keep the first row of each group, keep the first k", for COR_F32 / COR_BF16 / COR_F16,
 * every C that cor_similarity_topk accepts and 1 <= k <= COR_TOPK_KMAX. Other arguments and alignment as for cor_similarity_topk;
 * workspace >= cor_topk_distinct_workspace_bytes(Bq, Ng, k). A null row_groups, exactly one of the two label pointers null, or a
 * filter_mode that is neither COR_FILTER_EQ nor COR_FILTER_NE (also when unfiltered): COR_EINVAL.
 * Route: the wide route for every k. The sample pass keeps the ROW of every sampled value, the threshold kernel reduces the sampled values
 * to one per group id before it takes the k-th (tau_q is valid only if k DISTINCT groups have a row above it), the wide / filtered scan
 * appends the scores >= tau_q unchanged, and one block per query reduces the candidates to one per group, selects the k-th best group,
 * re-scores every candidate row within delta_q of it with the chain and keeps the first row of each group in rank order. An overflowed
 * query (thousands of rows of one group ahead of everything else, fewer than k groups in a large shard) is ranked on the device by paging
 * through the shard in rank order until k groups are found (exact; no host round trip). Flags: COR_TOPK_NO_FALLBACK keeps its meaning
 * (index -2 in every slot of an overflowed query); COR_TOPK_FORCE_LISTS and COR_TOPK_WAVE_FINAL return COR_ENOSUPPORT;
 * COR_TOPK_FORCE_GLOBAL_THRESHOLD has no effect.
 * Cost of the fallback: it pages through the shard 2048 rows at a time, five chain passes over the whole shard per page, until k groups
 * are found. A query that finds them in the first pages (thousands of near-identical rows) costs a few passes; a shard with FEWER THAN k
 * groups allowed for a query is paged to its end: Ng / 2048 pages x 5 Ng row scores = Ng^2 / 410 row scores per query in one block of 256
 * threads (2.4e7 at 100k rows, 2.4e9 at 1M rows: seconds). Such shards are legal and exact, but keep them small, or search them with
 * cor_similarity_topk_filtered per group.
 * cor_topk_distinct_sample_values: the most sample values per query any plan of this call shape hands the threshold kernel, which sorts
 * at most 4096 of them in LDS; the plan keeps it within that for every Ng (tests assert it; a plan that did not would be refused with
 * COR_ENOSUPPORT). With a filter, 16-bit C = 256 shards beyond ~23M rows at k = 256 (~60M at k = 100) pay for it with a wider sample
 * stride than the candidate buffers are planned for: their queries overflow into the fallback above. */
long cor_topk_distinct_workspace_bytes(int Bq, int Ng, int k);
int cor_topk_distinct_sample_values(int Bq, int Ng, int k);
int cor_similarity_topk_distinct(const float* Q, const void* G, int g_dtype, int Bq, int Ng, int C, int k, long long g_offset,
                                 const int* row_groups, const int* row_labels, const int* query_labels, int filter_mode, float* out_scores,
                                 long long* out_idx, void* workspace, int flags, void* stream);

/* Int8 galleries (a scalar-quantised index, "SQ8"): rows quantised per row to int8 with one fp32 scale, scanned on the i8 matrix cores.
 * ROW QUANTISATION (cor_quantize_rows_i8): X [n,C] in x_dtype (COR_F32 / COR_BF16 / COR_F16; 16-bit values widened exactly), finite
 * values -> q int8 [n,C], scale f32 [n]. Per row: amax = max_c |x_c| in fp32. amax == 0: scale = 0 and every q_c = 0. Otherwise
 *     inv = 127.0f / amax;   q_c = clamp((int)rintf(x_c * inv), -127, 127);   scale = amax / 127.0f
 * with every operation a separately rounded fp32 operation (no contraction, plain division, no fast-math) and rintf rounding half to
 * even. C % 16 == 0 and C <= 256, an x_dtype above: else COR_ENOSUPPORT; null pointers, n < 0, C <= 0, X or q not 16-byte aligned:
 * COR_EINVAL; n == 0 is a successful no-op. One launch, memory-bound (16 lanes per row, 16-byte loads and stores).
 * SCORE of query b against row g (cor_similarity_topk_i8): qq, qscale = the same quantisation of the fp32 query, made inside the call;
 *     d = sum_c qq[b,c] * Gq[g,c] in int32;   score = ((float)d * qscale[b]) * gscale[g]
 * two separately rounded fp32 multiplies. |d| <= 127^2 * C < 2^24 for C <= 256: (float)d is exact, d is exact in any summation order, so
 * the score has no error bound to carry: what the scan computes is the score.
 * ORDER: by the order-preserving key of the score's bits descending (so +0.0 ranks above -0.0, which a zero scale can produce), then by
 * row index ascending; out_scores f32 [Bq,k], out_idx i64 [Bq,k] = row + g_offset; Ng < k: the tail is (-inf, -1). The result is
 * bit-identical to that definition evaluated on the CPU (tests/i8_refs.py), scores and indices.
 * Q f32 [Bq,C], Gq int8 [Ng,C] and gscale f32 [Ng] 16-byte aligned, 1 <= k <= COR_TOPK_KMAX, C % 16 == 0, C <= 256, workspace (256-byte
 * aligned) >= cor_topk_i8_workspace_bytes(Bq, Ng, k). Checks in the order and with the codes of cor_similarity_topk: null pointers or
 * Bq / Ng / k <= 0: COR_EINVAL; k or C unsupported: COR_ENOSUPPORT; a flag other than COR_TOPK_NO_FALLBACK: COR_ENOSUPPORT; misaligned
 * pointers: COR_EINVAL. No allocation, no host synchronisation: the call can be captured in a graph.
 * Route, the same for every k: the wide route's steps with the fp32 gallery's selection (delta = 0, nothing re-scored). The queries are
 * quantised into the workspace; a strided sample scan keeps group maxima; tau_q is their k-th largest; the full scan appends the
 * (score, row) entries >= tau_q to private per-stream lists (no atomics); one block per query finds the exact k-th key, takes the rows at
 * or above it and sorts them. An overflowed query (e.g. thousands of identical rows) is ranked on the device by a brute force over the int8
 * scores of the whole shard (exact, slow, rare); with COR_TOPK_NO_FALLBACK it carries index -2 in every slot instead.
 * The scan (v_mfma_i32_16x16x64_i8): a block of 8 waves shares every 64-row gallery tile through LDS and each wave keeps the fragments of
 * its own 64 queries in registers, so up to 512 queries read the gallery from memory once. */
int cor_quantize_rows_i8(const void* X, int x_dtype, int n, int C, signed char* q, float* scale, void* stream);
long cor_topk_i8_workspace_bytes(int Bq, int Ng, int k);
int cor_similarity_topk_i8(const float* Q, const signed char* Gq, const float* gscale, int Bq, int Ng, int C, int k, long long g_offset,
                           float* out_scores, long long* out_idx, void* workspace, int flags, void* stream);

/* Filtered int8 search (cor_similarity_topk_i8_filtered): the top-k of the ALLOWED rows of an int8 gallery.
 * SCORE and ORDER are exactly those of cor_similarity_topk_i8: d = the int32 dot product of the quantised query and the row,
 * score = ((float)d * qscale) * gscale, ranked by the order-preserving key of the score's bits descending, then row index ascending.
 * ALLOWED rows are exactly those of cor_similarity_topk_filtered: row g is allowed for query b if query_labels[b] < 0 (unrestricted), or
 * COR_FILTER_EQ and row_labels[g] == query_labels[b], or COR_FILTER_NE and row_labels[g] != query_labels[b]. row_labels i32 [Ng]
 * (shard-local row g; 16-byte aligned), query_labels i32 [Bq]. Per query the result is the top-k of its allowed rows only: fewer than k
 * allowed rows give those first and then the (-inf, -1) tail, no allowed row gives only the tail. The result is bit-identical to that
 * definition evaluated on the CPU (tests/i8_filtered_refs.py), scores and indices.
 * Other arguments as for cor_similarity_topk_i8; workspace (256-byte aligned) >= cor_topk_i8_filtered_workspace_bytes(Bq, Ng, k). Checks in
 * the order and with the codes of cor_similarity_topk_i8: null pointers (the label pointers included) or Bq / Ng / k <= 0: COR_EINVAL;
 * filter_mode neither COR_FILTER_EQ nor COR_FILTER_NE: COR_EINVAL; k > COR_TOPK_KMAX, C > 256 or C % 16: COR_ENOSUPPORT; a flag other than
 * COR_TOPK_NO_FALLBACK: COR_ENOSUPPORT; Q, Gq, gscale or row_labels not 16-byte aligned, workspace not 256-byte aligned: COR_EINVAL. No
 * allocation, no host synchronisation: the call can be captured in a graph.
 * Route: the int8 route's steps with the filter inside them: a disallowed score is -inf before the sample's group values, the threshold
 * and the append decision. A tile's 64 row labels travel through LDS with its 64 row scales, each lane keeps the labels of its four
 * queries in registers. The sample keeps the four best allowed scores per group and the scan slices walk the gallery interleaved (slice s
 * takes tiles s, s + nsplit, ...), so a selective filter keeps its threshold and a class-sorted gallery does not crowd a few candidate
 * streams. An overflowed query is ranked over its allowed rows by the brute force over the int8 scores; with COR_TOPK_NO_FALLBACK it
 * carries index -2 in every slot instead. */
long cor_topk_i8_filtered_workspace_bytes(int Bq, int Ng, int k);
int cor_similarity_topk_i8_filtered(const float* Q, const signed char* Gq, const float* gscale, int Bq, int Ng, int C, int k,
                                    long long g_offset, const int* row_labels, const int* query_labels, int filter_mode,
                                    float* out_scores, long long* out_idx, void* workspace, int flags, void* stream);

/* Distinct-group int8 search (cor_similarity_topk_i8_distinct): the best row of each of the k best groups of an int8 gallery.
 * SCORE and ORDER are exactly those of cor_similarity_topk_i8: d = the int32 dot product of the quantised query and the row,
 * score = ((float)d * qscale) * gscale, ranked by the order-preserving key of the score's bits descending (+0.0 above -0.0), then row
 * index ascending. ALLOWED rows are exactly those of cor_similarity_topk_distinct: every row when row_labels and query_labels are both
 * NULL; both given: the COR_FILTER_EQ / COR_FILTER_NE rule of cor_similarity_topk_filtered (query_labels[b] < 0: unrestricted); exactly
 * one NULL: COR_EINVAL. Filter labels and group ids are separate vectors and may be the same memory.
 * GROUPS: row_groups i32 [Ng] (shard-local row g; 16-byte aligned); a negative id makes the row a group of its own. Per query, among its
 * allowed rows, a group's representative is its first row in the ORDER above, and the result is the k best representatives in that
 * order: out_scores f32 [Bq,k], out_idx i64 [Bq,k] = the representative ROWS (+ g_offset), so no group appears twice. Fewer than k groups
 * with an allowed row: those first, then the (-inf, -1) tail; no allowed row: only the tail. The result is bit-identical, scores and
 * indices, to "rank the allowed rows by the int8 definition, keep the first row of each group, keep the first k" evaluated on the CPU
 * (tests/i8_distinct_refs.py).
 * Other arguments as for cor_similarity_topk_i8; workspace (256-byte aligned) >= cor_topk_i8_distinct_workspace_bytes(Bq, Ng, k), which
 * covers the call with or without labels and never shrinks when Bq grows (size it once for the largest batch). Checks in
 * the order and with the codes of cor_similarity_topk_i8_filtered: null Q / Gq / gscale / row_groups / outputs / workspace, Bq / Ng / k
 * <= 0 or exactly one label pointer null: COR_EINVAL; filter_mode neither COR_FILTER_EQ nor COR_FILTER_NE (also when unfiltered):
 * COR_EINVAL; k > COR_TOPK_KMAX, C > 256 or C % 16: COR_ENOSUPPORT; a flag other than COR_TOPK_NO_FALLBACK: COR_ENOSUPPORT; Q, Gq, gscale,
 * row_groups or row_labels not 16-byte aligned, workspace not 256-byte aligned: COR_EINVAL. No allocation, no host synchronisation: the
 * call can be captured in a graph.
 * Route: the int8 route's steps with the distinct route's three changes. The sample scan keeps the ROW behind every sampled value (the
 * lane-quarter group's maximum, with a filter its four best allowed scores); the threshold kernel of cor_similarity_topk_distinct
 * reduces the sampled values to one per group id before it takes the k-th (delta = 0); the append scan is that of the plain / filtered
 * int8 call unchanged; one block per query reduces the candidates to one per group, finds the exact k-th group, sorts every candidate at
 * or above it and keeps the first row of each group (nothing is re-scored: the scan's score is the score). An overflowed query is ranked
 * on the device by the paging fallback of cor_similarity_topk_distinct over the int8 scores (its cost note applies: Ng^2 / 410 row
 * scores for a shard with fewer than k allowed groups); with COR_TOPK_NO_FALLBACK it carries index -2 in every slot instead.
 * cor_topk_i8_distinct_sample_values: the most sample values per query a plan of this call shape hands the threshold kernel; at most
 * 4096 for every Ng (4 streams x <= 256 sample slices x 4 values with a filter), and a plan beyond it would be refused with
 * COR_ENOSUPPORT. */
long cor_topk_i8_distinct_workspace_bytes(int Bq, int Ng, int k);
int cor_topk_i8_distinct_sample_values(int Bq, int Ng, int k);
int cor_similarity_topk_i8_distinct(const float* Q, const signed char* Gq, const float* gscale, int Bq, int Ng, int C, int k,
                                    long long g_offset, const int* row_groups, const int* row_labels, const int* query_labels, int filter_mode,
                                    float* out_scores, long long* out_idx, void* workspace, int flags, void* stream);

/* Merge of top-k lists on the device: per query b, P lists of kin entries (what P calls of cor_similarity_topk[_filtered|_distinct] over P
 * shards return, stacked) -> the k best entries of their union. scores f32 [P,Bq,kin], idx i64 [P,Bq,kin] (global row ids), groups NULL or
 * i32 [P,Bq,kin] (one group id per entry), all contiguous; out_scores f32 [Bq,k], out_idx i64 [Bq,k], out_groups NULL or i32 [Bq,k].
 * Plain merge (groups == NULL): the P*kin entries of a query are ordered by (score desc, index asc). An entry with idx < 0 is MISSING: it
 * ranks after every present entry whatever its score, while a present entry whose score is -inf still ranks ahead of the missing ones.
 * The first k go out; positions past the number of present entries hold (-inf, -1). out_groups, if given, is filled with -1.
 * Scores compare as floats (-0.0 and +0.0 tie and the index decides) and their bits are copied through unchanged; indices compare as full
 * 64-bit values (g_offset is a long long: ids above 2^32 are legal). Preconditions: scores are finite or -inf; no row id occurs twice among
 * one query's present entries (two equal (score, index) pairs keep the order of their positions in the stacked lists).
 * Distinct merge (groups != NULL): after the same ranking an entry is dropped if an earlier-ranked present entry of the same query has the
 * same NON-NEGATIVE group id (negative ids are never merged) and missing entries are dropped; the first k survivors go out, then the
 * (-inf, -1) tail. out_groups receives the survivors' group ids (-1 in the tail), so a merged list can itself be merged again: a merged
 * list is the (distinct) top-k of the union of its inputs.
 * Both modes agree bitwise, scores and indices, with merge_topk_host / merge_topk_distinct_host of cor_amd/retrieval.py on lists as the
 * searches return them (missing entries carry (-inf, -1)). Nothing is indexed with a missing entry's index or group value, which may be
 * arbitrary. One launch, one block per query: a bitonic sort in LDS of 8-byte keys (order-preserving score key | position; the index is
 * read through the position on ties), for distinct a second sort by (group id, rank) with head flags and a block scan.
 * 1 <= k <= COR_TOPK_KMAX, kin >= 1, P >= 1, Bq >= 0 and non-null scores / idx / out_scores / out_idx, else COR_EINVAL; Bq == 0 is a
 * successful no-op; P*kin > COR_MERGE_NMAX: COR_ENOSUPPORT (merge in rounds: retrieval.merge_topk_device). cor_merge_topk_workspace_bytes
 * reports the same errors as negative values, as cor_topk_workspace_bytes does; the kernel needs no scratch memory today, so it returns 0
 * for every supported shape and `workspace` may then be NULL. */
long cor_merge_topk_workspace_bytes(int P, int Bq, int kin, int k);
int cor_merge_topk(const float* scores, const long long* idx, const int* groups, int P, int Bq, int kin, int k, float* out_scores,
                   long long* out_idx, int* out_groups, void* workspace, void* stream);

/* Re-scoring of candidate lists (the second stage of a two-stage search): per query b a list of kin global row ids -> the chain score of
 * every listed row this shard holds, ranked, every id once, the first k. Q f32 [Bq,C]; G [Ng,C] in g_dtype (COR_F32 / COR_BF16 / COR_F16),
 * the shard's rows, global ids [g_offset, g_offset + Ng); cand i64 [Bq,kin], contiguous; out_scores f32 [Bq,k], out_idx i64 [Bq,k] (global
 * ids), out_pos NULL or i32 [Bq,k].
 * Entry j of query b is PRESENT if g_offset <= cand[b,j] < g_offset + Ng and no earlier position j' < j of the same query holds the same
 * id; every other entry (negative ids, ids of other shards, repeats) is MISSING: it is dropped, and no address is ever derived from an id
 * that has not passed the range test, so the ids may be arbitrary 64-bit values. The score of a present entry is the fmaf-chain score of
 * cor_similarity_topk (oracle/c/sim_chain.c): the row's stored values widened exactly to fp32, for a 16-bit gallery the query rounded
 * (nearest even) to the gallery dtype and widened back, acc = fmaf(row, query, acc) from 0 over k = 8c+i then 8c+4+i, c = 0 .. C/8-1,
 * i = 0 .. 3. Every entry is scored with plain fmaf in that order; there is no approximate pass. Present entries are ordered by (score
 * desc, global id asc); scores compare as floats (-0.0 and +0.0 tie and the id decides) and the first k go out with the score bits as
 * computed. out_pos, if given, receives the entry's position j in the input list (of a repeated id: its first occurrence), so that a
 * caller can carry group ids or coarse scores along. Positions past the number of present entries hold (-inf, -1, -1).
 * Hence re-scoring the list a search returned against the gallery it searched gives that list back bitwise, whatever the order of the
 * candidates; and the lists of several shards over disjoint id ranges, each re-scoring the same cand, merge (cor_merge_topk) into the
 * list of one shard over all the rows.
 * One launch, one block per query: the query in LDS, thread-per-candidate row gathers with 16-byte loads (four chains interleaved per
 * thread), then the ranking of cor_merge_topk (bitonic sort in LDS of 8-byte keys, the id read through the position on ties), a keep flag
 * where the rank before holds another id, and a block scan that places the first k survivors.
 * 1 <= k <= COR_TOPK_KMAX, kin >= 1, Ng >= 0, Bq >= 0 and non-null Q / cand / out_scores / out_idx (G too unless Ng == 0), else
 * COR_EINVAL; Bq == 0 is a successful no-op; kin > COR_MERGE_NMAX, C > 256 or C % 16 != 0, an unknown g_dtype: COR_ENOSUPPORT. All of
 * these are decided before any HIP call. Q and G 16-byte aligned as for the searches. cor_rescore_workspace_bytes reports the errors it can
 * see as negative values; the kernel needs no scratch memory today, so it returns 0 for every supported shape and `workspace` may then be
 * NULL. No host synchronisation, no allocation; everything runs on `stream`. */
long cor_rescore_workspace_bytes(int Bq, int kin, int k);
int cor_rescore_topk(const float* Q, const void* G, int g_dtype, int Bq, int Ng, int C, long long g_offset, const long long* cand, int kin,
                     int k, float* out_scores, long long* out_idx, int* out_pos, void* workspace, void* stream);

/* Query expansion (AQE, its weighted form alpha-QE) and, applied to gallery rows with query_weight = 0, database-side augmentation (DBA):
 * per query b the weighted sum of the first m rows its list names plus the weighted query, optionally L2-normalised.
 * Q f32 [Bq,C], may be NULL when query_weight == 0. seg_rows / seg_offset / seg_n / seg_dtype are HOST arrays of nseg entries: segment s
 * holds the rows with global ids [seg_offset[s], seg_offset[s] + seg_n[s]) at the DEVICE pointer seg_rows[s], contiguous [seg_n[s], C] in
 * seg_dtype[s] (COR_F32 / COR_BF16 / COR_F16; dtypes may differ between segments); the id ranges must be pairwise disjoint (the segments of
 * a GallerySet, or the one of a GalleryShard). The launcher copies the table into a by-value kernel argument: no device allocation, no
 * host-to-device copy, no host synchronisation; everything runs on `stream` and the call can be captured in a graph. scores f32 [Bq,kin]
 * and idx i64 [Bq,kin], contiguous, are lists as the searches, the merge and the re-scoring return them; only the first m entries of each
 * are used (1 <= m <= kin, m <= COR_TOPK_KMAX). out [Bq,C] in out_dtype (COR_F32 / COR_BF16 / COR_F16; the 16-bit forms are the f32 result
 * rounded to nearest-even). Rows and Q 16-byte aligned as for the searches.
 * Definition, fixed to the bit: every operation below is ONE IEEE fp32 operation, separately rounded, never contracted to an fma.
 *   1. v[c] = query_weight * Q[b,c]; with query_weight == 0: v[c] = +0 and Q is not read.
 *   2. for j = 0 .. m-1 IN THAT ORDER: id = idx[b,j] is PRESENT if some segment s has seg_offset[s] <= id < seg_offset[s] + seg_n[s] (the
 *      difference is taken in unsigned arithmetic behind the test id >= seg_offset[s]; no address is formed from an id that failed, so ids
 *      may be arbitrary 64-bit values). A missing entry contributes nothing and its score is never used. A present one:
 *      t = scores[b,j] > 0 ? scores[b,j] : +0 (NaN, -0.0 and negative scores give +0); w = 1, then alpha times w = w * t (alpha == 0:
 *      w = 1); x[c] = the stored row value widened exactly to fp32; v[c] = v[c] + (w * x[c]). The addition is performed even when
 *      w == 0, and an id that occurs twice is added twice.
 *   3. normalize != 0: s[c] = v[c] * v[c] for c < C and +0 for C <= c < 256; for h = 128, 64, .., 1: s[c] = s[c] + s[c+h] for all c < h;
 *      d = sqrt(s[0]), raised to 1e-12f if smaller; out[c] = v[c] / d. A query with nothing to sum gives a zero row.
 *   4. normalize == 0: out[c] = v[c].
 * The order is by list position and the tree is over the channel index, so the result does not depend on how many segments hold the rows,
 * on their order, on the dtype of rows that store the same values, or on the launch geometry: several segments give the bits of one
 * segment over the concatenated rows.
 * One launch, one wave per query and four queries per block; each lane owns four consecutive channels, so a row is one coalesced wave
 * load; the loads of up to 8 list entries are issued before the first add; no LDS, no scratch, no global workspace.
 * COR_EINVAL: a null scores / idx / out, a null segment array with nseg > 0, Bq < 0, kin < 1, m < 1, m > kin, alpha < 0, alpha > 8, nseg < 0,
 * C < 1, a negative seg_n, a null seg_rows[s] with seg_n[s] > 0, a bad out_dtype, Q == NULL with a non-zero weight. COR_ENOSUPPORT:
 * m > COR_TOPK_KMAX, nseg > COR_EXPAND_SEGMAX, C > 256 or C % 16 != 0, an unknown seg_dtype. All of these are decided before any HIP call.
 * Bq == 0 is a successful no-op; nseg == 0 is legal (every entry is missing). */
#define COR_EXPAND_SEGMAX 16
int cor_expand_queries(const float* Q, float query_weight, const void* const* seg_rows, const long long* seg_offset, const int* seg_n,
                       const int* seg_dtype, int nseg, const float* scores, const long long* idx, int Bq, int kin, int m, int C, int alpha,
                       int normalize, void* out, int out_dtype, void* stream);

/* Int8-only galleries: the list stages over quantised rows (Gq int8 [n,C] with scale f32 [n], as cor_quantize_rows_i8 makes them), so that
 * a gallery resident as int8 alone is re-scored, expanded, augmented and re-ranked without a float copy of its rows. The int32 dot product
 * is exact in any summation order and every floating-point step below is ONE separately rounded IEEE fp32 operation, never contracted, so
 * none of these calls carries an error bound: each is bit-identical to its definition evaluated on the CPU (tests/i8_list_refs.py). No
 * call allocates or synchronises with the host; each runs on `stream` and can be captured in a graph; all argument errors are decided
 * before any HIP call.
 *
 * cor_dequantize_rows_i8: the dequantised row, x[g,c] = (float)q[g,c] * scale[g], ONE rounded fp32 multiply, stored into X [n,C] as fp32
 * (x_dtype COR_F32) or rounded again, to nearest-even, to COR_BF16 / COR_F16: the 16-bit forms are the ROUNDED fp32 product rounded a second
 * time (what a conversion of the fp32 output gives), not the exact product rounded once. C % 16 == 0 and C <= 256, an x_dtype above: else
 * COR_ENOSUPPORT; null pointers, n < 0, C <= 0, X or q not 16-byte aligned, scale not 4-byte aligned: COR_EINVAL (the checks and their
 * order are those of cor_quantize_rows_i8); n == 0 is a successful no-op. One launch, memory-bound (16 lanes per row, 16-byte loads and
 * stores).
 *
 * cor_rescore_topk_i8: cor_rescore_topk over an int8 shard. Q f32 [Bq,C]; Gq int8 [Ng,C] and gscale f32 [Ng], the shard's rows, global ids
 * [g_offset, g_offset + Ng); cand i64 [Bq,kin], contiguous; out_scores f32 [Bq,k], out_idx i64 [Bq,k] (global ids), out_pos NULL or
 * i32 [Bq,k]. Entry j of query b is PRESENT if g_offset <= cand[b,j] < g_offset + Ng and no earlier position j' < j of the same query
 * holds the same id; every other entry (negative ids, ids of other shards, repeats) is MISSING: it is dropped, and no address is ever
 * derived from an id that has not passed the range test, so the ids may be arbitrary 64-bit values. The SCORE of a present entry is that
 * of cor_similarity_topk_i8: qq, qscale = the quantisation of the fp32 query by the rule of cor_quantize_rows_i8, made inside the call;
 * d = sum_c qq[b,c] * Gq[g,c] in int32; score = ((float)d * qscale[b]) * gscale[g], two separately rounded fp32 multiplies. Present
 * entries are ordered by (score desc, global id asc) with the list kernels' rules: scores compare as floats (-0.0 and +0.0 tie and the id
 * decides) and the first k go out with the score bits as computed. out_pos, if given, receives the entry's position j in the input list
 * (of a repeated id: its first occurrence). Positions past the number of present entries hold (-inf, -1, -1).
 * Hence re-scoring the list an int8 search returned against the gallery it searched gives that list back bitwise, whatever the order of
 * the candidates, with ONE exception: a list that holds both +0.0 and -0.0 scores (which needs row scales small enough for the product to
 * underflow, or hand-made scales of both signs). The search orders by the score's bits, so every +0.0 ranks before every -0.0; this call
 * compares them as equal and lets the id decide. The lists of several shards over disjoint id ranges, each re-scoring the same cand,
 * merge (cor_merge_topk, which has the same tie rule) into the list of one shard over all the rows.
 * One launch, one block per query: the first wave reduces the query's amax and writes the int8 query (C bytes) and qscale to LDS;
 * thread-per-candidate row gathers with 16-byte loads (a row is C bytes; four candidates interleaved per thread) feeding v_dot4c_i32_i8;
 * then the ranking, keep flags, block scan and tail of cor_rescore_topk.
 * 1 <= k <= COR_TOPK_KMAX, kin >= 1, Ng >= 0, Bq >= 0 and non-null Q / cand / out_scores / out_idx (Gq and gscale too unless Ng == 0),
 * else COR_EINVAL; then kin > COR_MERGE_NMAX, C > 256 or C % 16 != 0: COR_ENOSUPPORT (the order of cor_rescore_topk's checks); Bq == 0 is
 * a successful no-op. Q and Gq 16-byte aligned as for the searches. cor_rescore_i8_workspace_bytes reports the errors it can see as
 * negative values; the kernel needs no scratch memory, so it returns 0 for every supported shape and `workspace` may then be NULL.
 *
 * cor_expand_queries_sq: cor_expand_queries with one more HOST array, seg_scale: for a segment of seg_dtype COR_I8 (rows int8
 * [seg_n[s], C]) seg_scale[s] is the DEVICE pointer of its f32 [seg_n[s]] row scales (a null entry, or a null seg_scale, with seg_n[s] > 0
 * there: COR_EINVAL); for a float segment the entry is ignored and seg_scale may be NULL when no segment is COR_I8. Float and int8 segments
 * may stand in one table. The definition is that of cor_expand_queries with one added line in step 2: for a row of an int8 segment the
 * stored value widened to fp32 is x[c] = (float)q[c] * scale[row], ONE rounded fp32 multiply; then v[c] = v[c] + (w * x[c]) as before.
 * The result therefore equals bitwise the expansion over an fp32 segment that holds the dequantised rows (cor_dequantize_rows_i8), and
 * still does not depend on how the rows are cut into segments or on which dtype stores equal values. All other arguments, limits and
 * error codes are those of cor_expand_queries, an unknown seg_dtype (COR_I8 is known here) being COR_ENOSUPPORT; cor_expand_queries itself
 * keeps refusing COR_I8. Kernel: that of cor_expand_queries; the lane's four channels of an int8 row are ONE dword, so at C = 256 a row is
 * one 256-byte wave load, and the row's scale is fetched by the lane that looked the id up and travels with the weight by v_readlane. A
 * table without int8 rows runs cor_expand_queries' own kernels. */
int cor_dequantize_rows_i8(const signed char* q, const float* scale, int n, int C, void* X, int x_dtype, void* stream);
long cor_rescore_i8_workspace_bytes(int Bq, int kin, int k);
int cor_rescore_topk_i8(const float* Q, const signed char* Gq, const float* gscale, int Bq, int Ng, int C, long long g_offset,
                        const long long* cand, int kin, int k, float* out_scores, long long* out_idx, int* out_pos, void* workspace,
                        void* stream);
int cor_expand_queries_sq(const float* Q, float query_weight, const void* const* seg_rows, const float* const* seg_scale,
                          const long long* seg_offset, const int* seg_n, const int* seg_dtype, int nseg, const float* scores,
                          const long long* idx, int Bq, int kin, int m, int C, int alpha, int normalize, void* out, int out_dtype,
                          void* stream);

/* k-reciprocal re-ranking (Zhong et al., CVPR 2017), SET FORM: uniform weights and the Jaccard index of k-reciprocal neighbour sets, mixed
 * with the original score by lam. Not implemented: the paper's Gaussian weights, the 2/3-overlap set expansion, the local query expansion
 * over k2. Two entry points: the reciprocal pruning of a gallery's neighbour graph (once per gallery) and the re-ranking of lists.
 *
 * cor_knn_reciprocal. A neighbour graph is, per segment s of a gallery (global ids [seg_offset[s], seg_offset[s] + seg_n[s]), pairwise
 * disjoint, at most COR_RERANK_SEGMAX segments), a DEVICE array seg_nbr[s] i64 [seg_n[s], k1], contiguous: row g holds the global ids of
 * the k1 nearest rows of row g, as a search returns them (-1 where fewer exist). The segment arrays are HOST arrays of nseg entries and
 * travel by value in the kernel arguments. The call prunes segment `seg`: out i64 [seg_n[seg], k1], a buffer of its own (never one of the
 * inputs), receives out[g, j] = h = seg_nbr[seg][g, j] if h lies in some segment's id range AND the global id of row g,
 * seg_offset[seg] + g, occurs among the k1 ids of h's row; otherwise -1. The range test comes before any address is formed from h
 * (unsigned difference behind h >= seg_offset[s]), so the ids may be arbitrary 64-bit values. One thread per (g, j). A row that lists
 * itself keeps itself. COR_EINVAL: a null segment array, nseg < 1, k1 < 1, seg outside [0, nseg), a negative seg_n, a null seg_nbr[s] with
 * seg_n[s] > 0, a null out with seg_n[seg] > 0. COR_ENOSUPPORT: k1 > COR_TOPK_KMAX, nseg > COR_RERANK_SEGMAX. seg_n[seg] == 0 is a
 * successful no-op.
 *
 * cor_rerank_reciprocal. scores f32 [Bq,kin] and idx i64 [Bq,kin], contiguous: lists as the searches, the merge or the re-scoring return
 * them. Segment s of the graph: seg_rnbr[s] i64 [seg_n[s], kg] (the pruned lists above, kg the graph's width), seg_kth[s] f32 [seg_n[s]]
 * (the score of each row's k1-th neighbour; -inf where fewer than k1 rows exist), seg_offset[s], seg_n[s]; HOST arrays of nseg DEVICE
 * pointers, copied into a by-value kernel argument. out_scores f32 [Bq,k], out_idx i64 [Bq,k], out_pos NULL or i32 [Bq,k].
 * Definition, per query b, fixed to the bit:
 *   Entry j is PRESENT if idx[b,j] lies in some segment's [seg_offset[s], seg_offset[s] + seg_n[s]); the range test runs before any
 *   address is formed (unsigned difference behind id >= seg_offset[s]), so ids may be arbitrary 64-bit values. Every other entry is
 *   MISSING: it is dropped and its score is never read.
 *   Preconditions: the present entries of one query have pairwise different ids and finite scores; lam is finite. (If they do not hold
 *   the result is unspecified, but every access stays in bounds.)
 *   A = { idx[b,j] : j < k1, present, scores[b,j] >= kth[idx[b,j]] }: the query's k-reciprocal set. A gallery row counts the query among
 *   its k1 nearest if the query scores at least as high as the row's k1-th neighbour.
 *   For every present entry j (all kin positions): B_j = the non-negative ids among rnbr[idx[b,j], 0 .. kg) (counted by position: a
 *   graph built by a search names every id once, so these are set sizes); I = |A n B_j|; U = |A| + |B_j| - I;
 *   J = U > 0 ? float(I) / float(U) : +0;  f = (lam * scores[b,j]) + ((1.0f - lam) * J).
 *   Each of the five fp32 operations (two conversions aside, which are exact) is ONE separately rounded IEEE operation, never an fma.
 *   The present entries are ranked by (f desc, id asc) with cor_merge_topk's rules: -0.0 and +0.0 tie and the id decides; ids compare
 *   as 64-bit values. The first k go out with f's bits as computed; out_pos is the entry's position j; positions past the number of
 *   present entries hold (-inf, -1, -1). lam == 1 therefore returns the present entries ordered by (score desc, id asc), which for a
 *   list as a search returns it is the input order, with scores * 1 + 0 * J as scores.
 * One launch, one block per query: A is built and sorted in LDS; thread-per-candidate, each candidate's rnbr row is read from global
 * memory (16-byte loads for even kg) and every id is binary-searched in A; then cor_merge_topk's ranking (bitonic sort in LDS of 8-byte
 * keys [f key | position], the id read through the position on ties). No scratch, no allocation, no host synchronisation; everything
 * runs on `stream` and the call can be captured in a graph.
 * COR_EINVAL: a null scores / idx / out_scores / out_idx, Bq < 0, kin / kg / k1 / k < 1, k1 > kin, nseg < 0, a null segment array with
 * nseg > 0, a negative seg_n, a null seg_rnbr[s] or seg_kth[s] with seg_n[s] > 0. COR_ENOSUPPORT: kin > COR_MERGE_NMAX; k, k1 or
 * kg > COR_TOPK_KMAX; nseg > COR_RERANK_SEGMAX. All of these are decided before any HIP call. Bq == 0 is a successful no-op; nseg == 0 is
 * legal (every entry is missing). */
#define COR_RERANK_SEGMAX 16
int cor_knn_reciprocal(const long long* const* seg_nbr, const long long* seg_offset, const int* seg_n, int nseg, int k1, int seg,
                       long long* out, void* stream);
int cor_rerank_reciprocal(const float* scores, const long long* idx, const long long* const* seg_rnbr, const float* const* seg_kth,
                          const long long* seg_offset, const int* seg_n, int nseg, int Bq, int kin, int kg, int k1, float lam, int k,
                          float* out_scores, long long* out_idx, int* out_pos, void* stream);

/* Result diversification: greedy maximal marginal relevance (MMR; Carbonell & Goldstein, SIGIR 1998) over a candidate list, with optional
 * near-duplicate suppression. Per query, k times: the entry with the best mix of its score and its largest similarity to the entries
 * already chosen goes out; an entry that is at least max_sim similar to a chosen one leaves for good.
 *
 * cor_diversify_mmr. The segment table is that of cor_expand_queries_sq: seg_rows / seg_scale / seg_offset / seg_n / seg_dtype are HOST
 * arrays of nseg entries; segment s holds the rows with global ids [seg_offset[s], seg_offset[s] + seg_n[s]) at the DEVICE pointer
 * seg_rows[s], contiguous [seg_n[s], C] in seg_dtype[s] (COR_F32 / COR_BF16 / COR_F16 / COR_I8, mixed freely); for a COR_I8 segment
 * seg_scale[s] is the DEVICE pointer of its f32 [seg_n[s]] row scales, for a float segment the entry is ignored and seg_scale may be NULL
 * when no segment is COR_I8. At most COR_DIVERSIFY_SEGMAX segments with pairwise disjoint id ranges. The launcher copies the table into a
 * by-value kernel argument: no device allocation, no host-to-device copy, no host synchronisation; everything runs on `stream` and the call
 * can be captured in a graph. scores f32 [Bq,kin] and idx i64 [Bq,kin], contiguous: lists as the searches, the merge or the re-scoring
 * return them. out_scores f32 [Bq,k], out_idx i64 [Bq,k], out_pos NULL or i32 [Bq,k], out_value NULL or f32 [Bq,k]. Rows 16-byte aligned as
 * for the searches.
 * Definition, per query b, fixed to the bit:
 *   Presence. Entry j < kin is PRESENT if idx[b,j] lies in some segment's [seg_offset[s], seg_offset[s] + seg_n[s]); the range test runs
 *   before any address is formed (unsigned difference behind id >= seg_offset[s]), so ids may be arbitrary 64-bit values. Every other
 *   entry is MISSING: it is dropped and its score is never read. Ids may repeat; a repeat is an entry of its own, ranked by its position.
 *   Row value. x(r)[c] of an fp32 row is the stored value; of a bf16 / fp16 row the stored value widened exactly; of an int8 row
 *   (float)q[c] * scale[row], ONE rounded fp32 multiply (the rule of cor_expand_queries_sq).
 *   Similarity. sim(r, r') is the fmaf chain of oracle/c/sim_chain.c over x(r) and x(r'): acc = +0; for chunk c = 0 .. C/8 - 1 and
 *   i = 0 .. 3: acc = fmaf(x(r)[8c+i], x(r')[8c+i], acc), then acc = fmaf(x(r)[8c+4+i], x(r')[8c+4+i], acc). It is bitwise symmetric. For
 *   int8 rows this is on purpose NOT the int32 score of the int8 searches: the result must not depend on which dtype stores equal values
 *   or on how the rows are cut into segments.
 *   State. m_j = +0 for every present entry; all present entries start ALIVE.
 *   Step t = 0 .. k-1, while an entry is alive:
 *     1. for every alive entry f_j = (lam * scores[b,j]) - ((1.0f - lam) * m_j): four separately rounded IEEE fp32 operations, never
 *        contracted.
 *     2. the winner w is the alive entry with the greatest f, compared as floats (-0.0 and +0.0 tie); then the smaller 64-bit id wins,
 *        then the smaller position. The id is read only on a tie.
 *     3. output slot t: out_scores = the winner's INPUT score bits, unchanged (the list still feeds cor_expand_queries /
 *        cor_rerank_reciprocal); out_idx = its id; out_pos = its position j; out_value = f_w as computed.
 *     4. w leaves the alive set. For every remaining alive entry j: v = sim(row_j, row_w); if v > m_j then m_j = v (strict: the penalty
 *        is never negative and there is no +-0 ambiguity); if v >= max_sim the entry is SUPPRESSED and leaves the alive set for good.
 *        max_sim = +inf turns suppression off.
 *   Tail. Slots past the last winner hold (-inf, -1, -1, -inf).
 *   Preconditions: present entries have finite scores and rows. (Otherwise the result is unspecified, but every access stays in bounds.)
 * Consequences. lam = 1 with max_sim = +inf returns the present entries ordered by (score desc, id asc, position asc) with their score
 * bits: a list as a search returns it comes back unchanged. lam = 1 with a finite max_sim is greedy near-duplicate suppression in score
 * order. Several segments, or another storage dtype for the same values, give the bits of ONE fp32 segment over the concatenated widened
 * rows. max_sim = -inf gives exactly one output per query that has a present entry.
 * One launch, one block per query, max(64, min(npad, 256), npad / 4) threads (npad = kin rounded up to a power of two), one to four
 * candidates per thread with their state in registers. Each step is one block-wide argmax (wave butterfly, then the waves' bests through
 * LDS) and one similarity pass: the winner's row is widened into 1 KiB of LDS and every thread advances its alive candidates' chains
 * against it. A table of one storage dtype stages the rows through LDS, a wave copying 8 rows x 128 bytes per load into an image of its
 * own (9 KiB of dynamic LDS per wave) from which every lane reads its row back; a table of mixed dtypes gathers thread per candidate
 * with 16-byte loads, up to four chains interleaved. k * kin chains per query at most; no Gram matrix, no global workspace, no scratch.
 * COR_EINVAL: a null scores / idx / out_scores / out_idx, a null segment array (seg_rows, seg_offset, seg_n, seg_dtype) with nseg > 0,
 * Bq < 0, kin < 1, k < 1, nseg < 0, C < 1, a negative seg_n, a null seg_rows[s] with seg_n[s] > 0, a null scale (entry or array) for a
 * non-empty COR_I8 segment, lam NaN or outside [0, 1], max_sim NaN. COR_ENOSUPPORT: kin > COR_MERGE_NMAX, k > COR_TOPK_KMAX,
 * nseg > COR_DIVERSIFY_SEGMAX, C > 256 or C % 16 != 0, an unknown seg_dtype. All of these are decided before any HIP call. Bq == 0 is a
 * successful no-op; nseg == 0 is legal (every entry is missing). */
#define COR_DIVERSIFY_SEGMAX 16
int cor_diversify_mmr(const void* const* seg_rows, const float* const* seg_scale, const long long* seg_offset, const int* seg_n,
                      const int* seg_dtype, int nseg, const float* scores, const long long* idx, int Bq, int kin, int C, float lam,
                      float max_sim, int k, float* out_scores, long long* out_idx, int* out_pos, float* out_value, void* stream);

/* Diffusion re-ranking: manifold ranking (Zhou et al., NIPS 2003; Iscen et al., CVPR 2017, "Efficient diffusion on region manifolds") on the
 * mutual k-nearest-neighbour graph of a query's candidates. The scores of the query's best entries are spread along chains of mutually
 * close rows, so a row that is far from the query but linked to it through such a chain (another view or crop of the same object) rises.
 *
 * cor_rerank_diffusion. The segment table is exactly that of cor_diversify_mmr: seg_rows / seg_scale / seg_offset / seg_n / seg_dtype are
 * HOST arrays of nseg entries (COR_F32 / COR_BF16 / COR_F16 / COR_I8 segments, mixed freely, a COR_I8 segment with its DEVICE row scales;
 * seg_scale may be NULL when no segment is COR_I8), at most COR_DIFFUSE_SEGMAX segments with pairwise disjoint id ranges, copied into a
 * by-value kernel argument together with the scalars: no device allocation, no workspace, no host-to-device copy, no host
 * synchronisation; everything runs on `stream` and the call can be captured in a graph. scores f32 [Bq,kin] and idx i64 [Bq,kin],
 * contiguous: lists as the searches, the merge or the re-scoring return them. out_scores f32 [Bq,k], out_idx i64 [Bq,k], out_pos NULL or
 * i32 [Bq,k]. Rows 16-byte aligned as for the searches.
 * Definition, per query b, fixed to the bit: every * + - / and sqrtf below is ONE IEEE fp32 operation, correctly rounded, never
 * contracted; fmaf is one fused operation.
 *   Presence. Entry j < kin is PRESENT if idx[b,j] lies in some segment's [seg_offset[s], seg_offset[s] + seg_n[s]); the range test runs
 *   before any address is formed, so ids may be arbitrary 64-bit values. Every other entry is MISSING: it is dropped and its score is
 *   never read. Ids may repeat; a repeat is an entry of its own. n is the number of present entries, numbered p = 0 .. n-1 in list order.
 *   Row value and similarity. x(r) and sim(r, r') are exactly those of cor_diversify_mmr: values widened exactly, an int8 value
 *   (float)q * scale as one rounded multiply, sim the fmaf chain of oracle/c/sim_chain.c, bitwise symmetric. The result depends neither
 *   on the storage dtype of equal values nor on how the rows are cut into segments.
 *   Power. pw(v) = +0 if !(v > 0); otherwise w = v, then w = w * v repeated gamma - 1 times. No powf.
 *   Affinity. a(p, p') = pw(sim(row_p, row_p')) for p != p' (by position, not by id: two entries with one id are neighbours); a(p, p) = 0.
 *   Neighbours. N(p): the at most kd entries p' with the greatest a(p, p') > 0, ordered by (a desc, p' asc). M(p): the members p' of
 *   N(p) with p in N(p'), the order kept: the mutual k-nearest-neighbour graph, symmetric because sim is.
 *   Degree. d_p = +0, then d_p = d_p + a(p, p') over M(p) in that order. Scale. r_p = d_p > 0 ? 1.0f / sqrtf(d_p) : +0.
 *   Edge weight. S(p, p') = a(p, p') * (r_p * r_p'), the inner product first.
 *   Query vector. y_p = p < kq ? pw(scores[b, position of p]) : +0: only the query's kq best present entries inject mass; kq >= n: all.
 *   Iteration. f(0) = y. For t = 0 .. iters-1 and every p: g = +0, then g = fmaf(S(p, p'), f(t)_p', g) over M(p) in its order;
 *   f(t+1)_p = (alpha * g) + ((1.0f - alpha) * y_p). All of f(t+1) is computed from f(t) (Jacobi).
 *   Ranking. The present entries are ranked by (f(iters) desc, id asc, position asc) with cor_merge_topk's rules: -0.0 ties with +0.0,
 *   ids compare as 64-bit values. The first k go out: out_scores = f's bits, out_idx = the id, out_pos = the list position j. Slots
 *   past n hold (-inf, -1, -1).
 *   Preconditions: present entries have finite scores and rows. (Otherwise the result is unspecified, but every access stays in bounds.)
 * Consequences. alpha = 0 returns y exactly: with gamma = 1 and kq >= n a searched list with positive scores comes back unchanged.
 * kd >= n - 1 makes M(p) every p' with a(p, p') > 0. A row with no positive similarity to any other row keeps f = (1 - alpha) * y
 * after the first step (as (alpha * 0) + that). n = 1 returns the entry with f = (alpha * 0) + ((1 - alpha) * y). f is never negative
 * and never -0.0.
 * One launch, one block per query, max(64, kin rounded up to a power of two) threads, one per candidate; all n * n chains are computed,
 * 32 partner rows at a time: the block widens the partners into an LDS tile, every thread walks its own row 8 channels at a time against
 * 32 accumulators and keeps its kd best affinities as a sorted list, in registers for kd <= 8, as a column in LDS for a larger kd (which is
 * several times slower: DESIGN.md). The mutual test needs only each list's last pair. The
 * iteration runs over two f vectors in LDS, a barrier per step; the ranking is cor_merge_topk's (bitonic sort in LDS of 8-byte keys
 * [f key | position], the id read through the position on ties). No Gram matrix, no global workspace, no scratch.
 * COR_EINVAL: a null scores / idx / out_scores / out_idx, a null segment array (seg_rows, seg_offset, seg_n, seg_dtype) with nseg > 0,
 * Bq < 0, kin / k / kd / kq / gamma / iters < 1, nseg < 0, C < 1, a negative seg_n, a null seg_rows[s] with seg_n[s] > 0, a null scale
 * (entry or array) for a non-empty COR_I8 segment, alpha NaN or outside [0, 1). COR_ENOSUPPORT: kin > COR_DIFFUSE_NMAX,
 * kd > COR_DIFFUSE_KDMAX, gamma > 4, iters > 64, k > COR_TOPK_KMAX, nseg > COR_DIFFUSE_SEGMAX, C > 256 or C % 16 != 0, an unknown
 * seg_dtype. All of these are decided before any HIP call. Bq == 0 is a successful no-op; nseg == 0 is legal (every entry is missing). */
#define COR_DIFFUSE_NMAX 256     /* candidates per query */
#define COR_DIFFUSE_KDMAX 32     /* graph neighbours per candidate */
#define COR_DIFFUSE_SEGMAX 16
int cor_rerank_diffusion(const void* const* seg_rows, const float* const* seg_scale, const long long* seg_offset, const int* seg_n,
                         const int* seg_dtype, int nseg, const float* scores, const long long* idx, int Bq, int kin, int C,
                         int kd, int kq, int gamma, float alpha, int iters, int k,
                         float* out_scores, long long* out_idx, int* out_pos, void* stream);

/* Fusion of ranked lists: reciprocal-rank fusion (RRF; Cormack, Clarke & Buettcher, SIGIR 2009), CombSUM and CombMAX (Fox & Shaw, TREC-2
 * 1994). Per query, P rankings of the SAME request over the SAME global id space (several shots or views of one request, or several
 * galleries over one id space) become one ranking with one entry per distinct id. cor_merge_topk is not this: it ranks entries, not rows,
 * and keeps a row that two lists name twice.
 *
 * cor_fuse_lists. scores f32 [P,Bq,kin] and idx i64 [P,Bq,kin], contiguous, stacked like cor_merge_topk's: lists as the searches, the merge,
 * the re-scoring or any other stage return them. weights_host: P HOST floats, copied into a by-value kernel argument together with the
 * switches: no device allocation, no host-to-device copy, no host synchronisation; everything runs on `stream` and the call can be
 * captured in a graph. out_scores f32 [Bq,k], out_idx i64 [Bq,k], out_count NULL or i32 [Bq,k].
 * Definition, per query b, fixed to the bit: every + - * / below is ONE IEEE fp32 operation, separately rounded, never contracted.
 *   Valid entries. Entry e of list p is a HOLE if idx[p,b,e] < 0 or its score is not finite (exponent bits all ones: +-inf and NaN; a
 *   present entry with such a score is a hole too). Among the entries of ONE list that are no holes and carry the same id, only the one
 *   at the lowest position is VALID; the others are repeats and count for nothing. The RANK of an entry is its 0-based position e + 1:
 *   holes and repeats take ranks, so for lists as the stages return them this is the usual rank. Nothing is indexed with an id.
 *   Statistics. mn_p and mx_p are the least and the greatest score over the valid entries of list p, a -0.0 counting as +0.0 (neither is
 *   ever -0.0). A list with no valid entry has none and contributes nothing to any id, in any mode.
 *   Value of a valid entry with score s: normalize == COR_FUSE_NORM_NONE: v = s. COR_FUSE_NORM_MINMAX: v = (s - mn_p) / (mx_p - mn_p), two
 *   subtractions and one division; mx_p == mn_p: v = 1.0f.
 *   Contribution c_p of list p to an id:
 *     COR_FUSE_RRF: c = w_p / (rrf_c + (float)rank), one add and one divide, for a list that holds the id (has a valid entry with it);
 *       any other list contributes nothing. normalize / missing must be NONE / ZERO.
 *     COR_FUSE_SUM: c = w_p * v for a list that holds the id. A list that does not: nothing under COR_FUSE_MISSING_ZERO; under
 *       COR_FUSE_MISSING_FLOOR c = w_p * f_p with f_p = mn_p (NORM_NONE) or 0.0f (NORM_MINMAX): the best score the absent row could still
 *       have in a truncated sorted list.
 *     COR_FUSE_MAX: c = w_p * v for the lists that hold the id; the others are ignored. missing must be ZERO.
 *   Fused score. RRF and SUM: acc = +0.0f, then acc = acc + c_p for p = 0 .. P-1 in that order, over the lists that contribute.
 *     MAX: acc = the c of the first list (lowest p) that holds the id, then `if (c_p > acc) acc = c_p` for the further holding lists in
 *     ascending p: no fmaxf, so +-0 are decided by the order.
 *   Output. One entry per distinct id that is valid in at least one list, ranked by (fused score desc, id asc) with cor_merge_topk's rules:
 *   scores compare as floats, -0.0 ranks as +0.0 and its bits are preserved, ids compare as 64-bit values. The first k go out with the
 *   fused bits as computed; out_count receives the number of lists that hold the id (CombMNZ is count * the SUM output). Positions past
 *   the number of distinct ids hold (-inf, -1, -1). The order among ids whose fused score is NaN (weights large enough to overflow) is
 *   unspecified.
 * Consequences. P = 1, SUM, weight 1, NONE, ZERO returns a searched list as it is, except that a -0.0 score comes back as +0.0 (acc
 * starts at +0.0). A fused list is not a list that can be fused again exactly (ranks and statistics are those of the inputs): there
 * are no rounds, and everything must fit one launch.
 * One launch, one block per query: a bitonic sort in LDS of 16-bit position keys by (id, position) with the 64-bit ids held in LDS,
 * per-list min / max by wave reductions where the mode needs them, the thread at the head of every run of equal ids accumulating its run
 * in list order, and cor_merge_topk's ranking (8-byte keys [fused score key | slot], the id read on ties) of the heads. 19 bytes of LDS
 * per padded entry, 76 KB at 4096 entries; no scratch, no global workspace.
 * COR_EINVAL: a null scores / idx / weights_host / out_scores / out_idx; P < 1, Bq < 0, kin < 1, k < 1; an unknown mode / normalize /
 * missing; RRF with normalize != NONE or missing != ZERO; MAX with missing != ZERO; under RRF rrf_c not finite or < 0; a weight that
 * is not finite (the weights are read once P <= COR_FUSE_PMAX is known). COR_ENOSUPPORT: P > COR_FUSE_PMAX, P*kin > COR_MERGE_NMAX,
 * k > COR_TOPK_KMAX. All of these are decided before any HIP call. Bq == 0 is a successful no-op. cor_fuse_lists_workspace_bytes reports
 * the shape errors as negative values; the kernel needs no scratch memory, so it returns 0 for every supported shape and `workspace` may
 * then be NULL. */
#define COR_FUSE_PMAX 16
#define COR_FUSE_RRF 0
#define COR_FUSE_SUM 1
#define COR_FUSE_MAX 2
#define COR_FUSE_NORM_NONE 0
#define COR_FUSE_NORM_MINMAX 1
#define COR_FUSE_MISSING_ZERO 0
#define COR_FUSE_MISSING_FLOOR 1
long cor_fuse_lists_workspace_bytes(int P, int Bq, int kin, int k);
int cor_fuse_lists(const float* scores, const long long* idx, int P, int Bq, int kin, const float* weights_host, int mode, int normalize,
                   int missing, float rrf_c, int k, float* out_scores, long long* out_idx, int* out_count, void* workspace, void* stream);

/* Clustering of a gallery: spherical k-means (Dhillon & Modha, Machine Learning 2001) with farthest-point ("max-min") seeding (Gonzalez,
 * Theoretical Computer Science 1985). The cluster of a row is an id like any other: as `groups` of a distinct search it gives k results
 * from k modes of the gallery, as `labels` of a filtered search it confines a query to the cell of its nearest centre, and the centres are
 * the coarse quantiser of a cell-probing search. The ASSIGNMENT step is the existing search (the centres as an fp32 gallery, the rows as
 * queries, k = 1); these two calls are the seeding and the centre step. Both are defined to the bit.
 *
 * Common to both calls. The segment table is exactly that of cor_diversify_mmr: seg_rows / seg_scale / seg_offset / seg_n / seg_dtype are
 * HOST arrays of nseg entries (COR_F32 / COR_BF16 / COR_F16 / COR_I8 segments, mixed freely, a COR_I8 segment with its DEVICE row scales;
 * seg_scale may be NULL when no segment is COR_I8), at most COR_CLUSTER_SEGMAX segments with pairwise disjoint id ranges, copied into a
 * by-value kernel argument. Rows 16-byte aligned as for the searches. A row's VALUE x(r)[c] is the stored value widened exactly to fp32; of
 * an int8 row (float)q[c] * scale[row], ONE rounded fp32 multiply (the rule of cor_expand_queries_sq). n_total is the sum of seg_n.
 * C <= 256 and C % 16 == 0; 1 <= K <= COR_KMEANS_KMAX; n_total < 2^31. The calls make no device allocation, no host-to-device copy and no
 * host synchronisation; everything runs on `stream` and both calls can be captured in a graph. `workspace`: device memory of at least
 * cor_kmeans_workspace_bytes(n_total, K, C) bytes, 256-byte aligned, contents free; the figure covers both calls (they may share the buffer
 * when they do not run concurrently).
 * Error order, both calls; all of it is decided before any HIP call. (1) COR_EINVAL: a null output or workspace pointer (cor_kmeans_update:
 * out_score_sum NULL while seg_score is not, or the reverse); nseg < 0, K < 1, C < 1; a null segment array (seg_rows, seg_offset, seg_n,
 * seg_dtype; cor_kmeans_update: seg_assign) with nseg > 0. (2) COR_ENOSUPPORT: nseg > COR_CLUSTER_SEGMAX (before the arrays are read).
 * (3) COR_EINVAL: a negative seg_n; for a segment with seg_n > 0 a null seg_rows[s], a null scale (entry or array) of a COR_I8 segment, a
 * null seg_assign[s], a null seg_score[s] while seg_score is given. (4) COR_ENOSUPPORT: K > COR_KMEANS_KMAX, C > 256 or C % 16 != 0,
 * n_total >= 2^31, then an unknown seg_dtype. (5) cor_kmeans_seed only, COR_EINVAL: K > n_total, then a first_id that no segment holds.
 * cor_kmeans_workspace_bytes returns the byte count, or COR_EINVAL (n_total < 0, K < 1, C < 1), then COR_ENOSUPPORT (as in (4)).
 *
 * cor_kmeans_seed: K rows that are far from each other, deterministic, no random numbers. out_ids i64 [K], out_centroids f32 [K,C].
 * Definition, fixed to the bit:
 *   sim(r, r') is the fmaf chain of oracle/c/sim_chain.c over x(r) and x(r') (neither re-rounded): acc = +0; for chunk c = 0 .. C/8 - 1 and
 *   i = 0 .. 3: acc = fmaf(x(r)[8c+i], x(r')[8c+i], acc), then acc = fmaf(x(r)[8c+4+i], x(r')[8c+4+i], acc). It is bitwise symmetric.
 *   c_0 = the row with global id first_id. best[g] = -inf for every row g. For t = 0 .. K-1:
 *     1. out_ids[t] = the id of c_t, out_centroids[t,:] = x(c_t).
 *     2. for every row g: s = sim(c_t, g); if (s > best[g]) best[g] = s.
 *     3. c_t is CHOSEN.
 *     4. c_{t+1} = the row that is not chosen with the smallest best by the IEEE `<` comparison (-0.0 and +0.0 tie); ties go to the
 *        smallest global id.
 *   Preconditions: finite rows. (Otherwise the result is unspecified, but every access stays in bounds.)
 * The result depends only on the set of (id, value) pairs: not on how the rows are cut into segments, on the segments' order, on which
 * dtype stores equal values, or on the launch geometry ((best, id) is a total order on the rows). Identical rows are chosen last: a twin
 * of a chosen row has best = sim(r, r), the largest value a unit row reaches.
 * 2K launches: one that sets best and the first row, then per step a scoring launch (at most 4096 blocks of 256 threads; a thread owns
 * rows and walks their chains against c_t's row in LDS, keeps the smallest (best, id) it saw; one partial per block) and a one-block
 * launch that reduces the partials, marks the winner and leaves it ON THE DEVICE for the next step; the last step only writes its output.
 *
 * cor_kmeans_update: the centre step. seg_assign: a HOST array of nseg DEVICE pointers, int32 [seg_n[s]], the cluster of each row.
 * seg_score: NULL, or the same shape in f32: each row's score to its centre. prev: NULL or f32 [K,C]. out_centroids f32 [K,C], out_count
 * i32 [K], out_score_sum f32 [K], NULL exactly when seg_score is.
 * Definition, fixed to the bit: every + * / and sqrtf is ONE IEEE fp32 operation, correctly rounded, never contracted.
 *   Membership. The members of cluster c are the rows with assign == c, in ASCENDING GLOBAL ID. A row whose assign value lies outside
 *   [0, K) (-1, K, INT_MIN) belongs to no cluster; nothing but its assign entry is read.
 *   Chunk sums. The members are taken in chunks of 256 consecutive members by ordinal. For chunk j: p_j[ch] = +0, then
 *   p_j[ch] = p_j[ch] + x(member)[ch] in member order.
 *   Total. v[ch] = +0, then v[ch] = v[ch] + p_j[ch] for j ascending. The two-level order is part of the definition: it lets a large
 *   cluster be summed by several waves while the bits stay fixed.
 *   Normalisation. Exactly step 3 of cor_expand_queries: s[ch] = v[ch] * v[ch] for ch < C and +0 for C <= ch < 256; for h = 128, 64, ..,
 *   1: s[ch] = s[ch] + s[ch + h] for ch < h; d = max(sqrtf(s[0]), 1e-12f); out_centroids[c,ch] = v[ch] / d.
 *   Counts and score sums. out_count[c] = the number of members. out_score_sum[c]: the same two-level sum over the members' scores
 *   (q_j = +0, q_j = q_j + score in member order; then +0 plus the q_j for j ascending).
 *   Empty cluster. out_centroids[c,:] = prev[c,:] bit for bit, or +0 if prev is NULL; out_count[c] = 0, out_score_sum[c] = +0.
 *   Preconditions: finite rows and scores. prev and out_centroids must not overlap.
 * The result does not depend on how the rows are cut into segments, on the segments' order or on which dtype stores equal values.
 * n_total == 0 (also nseg == 0) is legal: every cluster is empty.
 * 6 launches. The member lists are built in the workspace by a stable counting sort: rows in tiles of 2048 (ascending id); per tile a
 * block sorts 32-bit keys [cluster | position in the tile] in LDS and writes the tile's count of every cluster into a tiles x K table;
 * one thread per cluster scans its column; one block scans the K totals; per tile a block places its rows. No atomics, integer or
 * float. Then one WAVE per (cluster, chunk): lane l owns channels [4l, 4l + 4), a member row is one coalesced wave load, eight loads are in
 * flight before the first add; the partial rows go to the workspace and one wave per cluster adds them up and normalises. */
#define COR_CLUSTER_SEGMAX 16
#define COR_KMEANS_KMAX 16384
long cor_kmeans_workspace_bytes(long n_total, int K, int C);
int cor_kmeans_seed(const void* const* seg_rows, const float* const* seg_scale, const long long* seg_offset, const int* seg_n,
                    const int* seg_dtype, int nseg, int C, int K, long long first_id, long long* out_ids, float* out_centroids,
                    void* workspace, void* stream);
int cor_kmeans_update(const void* const* seg_rows, const float* const* seg_scale, const long long* seg_offset, const int* seg_n,
                      const int* seg_dtype, int nseg, const int* const* seg_assign, const float* const* seg_score, int C, int K,
                      const float* prev, float* out_centroids, int* out_count, float* out_score_sum, void* workspace, void* stream);

/* Cell-probing search ("IVF-flat", Sivic & Zisserman ICCV 2003; Jegou, Douze & Schmid TPAMI 2011 without the product quantiser): the rows
 * of a gallery are laid out cell by cell after a clustering, a query names the cells whose centres it scores best against (its PROBES: an
 * exact search over the centres, made by the caller) and only those cells' rows are scored. The result is the EXACT top-k of those rows.
 * Both calls make no device allocation, no host-to-device copy and no host synchronisation, run on `stream` and can be captured in a graph.
 *
 * cor_ivf_build: a segment table and a per-row cell id -> cell-contiguous storage. The table is that of cor_kmeans_update (seg_rows /
 * seg_scale / seg_offset / seg_n / seg_dtype, nseg <= COR_CLUSTER_SEGMAX, pairwise disjoint id ranges) and seg_assign as it takes it: a HOST
 * array of nseg DEVICE pointers, int32 [seg_n[s]]. dtype: COR_F32 / COR_BF16 / COR_F16 / COR_I8, the dtype of the index AND of every
 * segment: rows are copied bit for bit, never converted. out_rows [n_total,C] in dtype (16-byte aligned), out_scale f32 [n_total] (required
 * for COR_I8, ignored otherwise), out_ids i64 [n_total], out_cell_start i32 [K+1].
 * Definition. The members of cell c are the rows with assign == c in ASCENDING GLOBAL ID (the member order of cor_kmeans_update). A row
 * whose assign value lies outside [0, K) (-1, K, INT_MIN) is in no cell and is not indexed; nothing but its assign entry is read.
 * cell_start[c] = the number of members of the cells < c; cell_start[K] = the number of indexed rows. The member with ordinal j of cell c
 * goes to slot cell_start[c] + j: its stored row bits, its scale (COR_I8) and its global id. Slots >= cell_start[K] are not written. The
 * result does not depend on how the rows are cut into segments or on the segments' order. n_total == 0 (also nseg == 0) is legal: every
 * entry of cell_start is 0.
 * Error order; all of it is decided before any HIP call. (1) COR_EINVAL: a null out_rows / out_ids / out_cell_start / workspace, a null
 * out_scale with dtype COR_I8; nseg < 0, K < 1, C < 1; a null segment array with nseg > 0. (2) COR_ENOSUPPORT: nseg > COR_CLUSTER_SEGMAX.
 * (3) COR_EINVAL: a negative seg_n; for a segment with rows a null seg_rows[s], scale or seg_assign[s]. (4) COR_ENOSUPPORT: K >
 * COR_KMEANS_KMAX, C > 256 or C % 16 != 0, n_total >= 2^31, an unknown seg_dtype; then an unknown dtype, then a segment (an empty one
 * included) of another dtype. (5) COR_EINVAL: out_rows or a segment's rows not 16-byte aligned, workspace not 256-byte aligned.
 * workspace >= cor_ivf_build_workspace_bytes(n_total, K, C) bytes (or COR_EINVAL for n_total < 0, K < 1, C < 1, then COR_ENOSUPPORT as (4)).
 * 5 launches: the stable counting sort of cor_kmeans_update (tile keys, column scan, scan, place; no atomics), then a copy in which one
 * wave moves a row with one coalesced load and one coalesced store.
 *
 * cor_ivf_search: Q f32 [Bq,C]; the index: rows [n,C] in dtype, scale f32 [n] (COR_I8; else ignored), ids i64 [n], cell_start i32 [K+1] as
 * cor_ivf_build wrote them; probes i64 [Bq,nprobe] contiguous, exactly what a search over the centres returns, 1 <= nprobe <=
 * COR_IVF_NPROBE_MAX; 1 <= k <= COR_TOPK_KMAX. out_scores f32 [Bq,k], out_idx i64 [Bq,k], out_scanned i32 [Bq] or NULL.
 * Definition. P(b) = the set of distinct values c in probes[b,:] with 0 <= c < K; every other value is ignored (-1 tails, repeats,
 * arbitrary 64-bit values: no address is formed from a probe that has not passed the range test). Cand(b) = the slots of the cells in
 * P(b); out_scanned[b] = |Cand(b)|.
 *   SCORE, float dtypes: the fmaf chain of cor_similarity_topk (acc = +0; for chunk c = 0 .. C/8 - 1 and i = 0 .. 3: acc = fmaf(x[8c+i],
 *   q[8c+i], acc), then acc = fmaf(x[8c+4+i], q[8c+4+i], acc): oracle/c/sim_chain.c), x the stored values widened exactly, q the query,
 *   rounded to the row dtype and widened back for 16-bit rows. COR_I8: the score of cor_similarity_topk_i8: the query quantised inside the
 *   call by the rule of cor_quantize_rows_i8, d the int32 dot product (exact), score = ((float)d * qscale) * scale[slot], two separately
 *   rounded multiplies.
 *   ORDER: that dtype's exact search with the global id ids[slot] in place of the row index. Float dtypes: score descending as floats
 *   (-0.0 and +0.0 tie), then id ascending; score bits are carried through unchanged. COR_I8: the order-preserving key of the score's BITS
 *   descending (+0.0 above -0.0), then id ascending. The first k entries go out, then the (-inf, -1) tail.
 * Equivalently: the lists equal bit for bit those of cor_similarity_topk / cor_similarity_topk_i8 run over a gallery that holds exactly
 * the candidate rows in ascending global id, indices mapped back to global ids; with every cell probed this is the exact search of the
 * indexed rows. Preconditions: finite rows; the ids of the index are pairwise distinct.
 * max_cell (>= 1: the largest cell's size, a HINT) and split (0: automatic; > 0: that many partial lists per query) change only how the work
 * is dealt out: any max_cell >= 1 and any legal split give the same bits. A cell larger than max_cell is still scanned to its end.
 * Error order; all of it is decided before any HIP call. (1) COR_EINVAL: a null Q / rows / ids / cell_start / probes / out_scores /
 * out_idx / workspace, a null scale with dtype COR_I8; Bq < 0; K, C, k, nprobe or max_cell < 1; split < 0. (2) COR_ENOSUPPORT: k >
 * COR_TOPK_KMAX, nprobe > COR_IVF_NPROBE_MAX, K > COR_KMEANS_KMAX, C > 256 or C % 16 != 0; split * k > COR_MERGE_NMAX; an unknown dtype.
 * (3) COR_EINVAL: Q or rows not 16-byte aligned, workspace not 256-byte aligned. Bq == 0 is a successful no-op. workspace >=
 * cor_ivf_search_workspace_bytes(Bq, K, C, nprobe, k, split) bytes, the same `split` as the call's (the query reports (1) and (2) as
 * negative values; it covers every max_cell).
 * 2 launches. Scan: the work units of a query are (probe j, slice s of its cell), S = ceil(max_cell / 512) slices per cell, slice s
 * walking the tiles s, s + S, ... of 512 slots; they are dealt round-robin to P blocks per query (automatic: P = min(ceil(1024 / Bq),
 * COR_MERGE_NMAX / k, the number of units)). A block keeps the query in LDS, a thread scores two rows at a time, reading each in whole
 * 128-byte lines, with plain interleaved fmaf chains (int8: 4-way integer dot products), and the block carries ONE running top-k in LDS:
 * after the first k rows the k-th key is a threshold, only rows at or above it are appended, and the buffer is sorted again (bitonic
 * network, ties by the id) when a tile might not fit. A probe is dropped inside the kernel if an earlier probe names the same cell.
 * Every block writes one partial list of k. Finish: one block per query ranks the P lists by the same order. (score, id) is a total
 * order on a query's candidates, so P, S and the order of the appends cannot show in the result. */
#define COR_IVF_NPROBE_MAX 256
long cor_ivf_build_workspace_bytes(long n_total, int K, int C);
int cor_ivf_build(const void* const* seg_rows, const float* const* seg_scale, const long long* seg_offset, const int* seg_n,
                  const int* seg_dtype, int nseg, const int* const* seg_assign, int C, int K, int dtype, void* out_rows, float* out_scale,
                  long long* out_ids, int* out_cell_start, void* workspace, void* stream);
long cor_ivf_search_workspace_bytes(int Bq, int K, int C, int nprobe, int k, int split);
int cor_ivf_search(const float* Q, const void* rows, const float* scale, int dtype, const long long* ids, const int* cell_start, int K, int C,
                   int Bq, const long long* probes, int nprobe, int k, int max_cell, int split, float* out_scores, long long* out_idx,
                   int* out_scanned, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* COR_AMD_H */
