/* arp_hip.h -- C ABI of libarp_hip.so: MI355X (gfx950) hot paths of ARP-DT.
 *
 * The reference (csmile-1006/ARP) is pure Python and has no FFI; the two hot paths are Python
 * closures.  Each entry point below names the reference seam it replaces (paths relative to
 * /root/reference).  INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions: every function returns 0 on success and a negative value on error; the message is
 * available from arp_last_error() (thread-local).  The caller owns every host buffer.  The library
 * owns device memory behind opaque handles.  A handle is bound to one HIP device and one HIP
 * stream and is NOT thread-safe (one host thread / process per GPU, as the reference's
 * single-threaded callers).  Calls are synchronous on return unless the name ends in _async.
 * There is NO CPU fallback: without a usable GPU every compute entry point fails.
 */
#ifndef ARP_HIP_H
#define ARP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARP_MODE_F32 0  /* parity mode: f32 storage, f32-input MFMA (exact f32 FMA chains)        */
#define ARP_MODE_BF16 1 /* throughput mode: bf16 GEMM operands, f32 accumulate/residual/LN/softmax */
#define ARP_MODE_F16 2  /* IEEE binary16 GEMM operands (same MFMA rate as bf16, 11 significand bits -- what openai/CLIP itself runs on a
                           GPU), everything else as BF16.  The DEFAULT throughput mode of every handle
                           (arp_clip, arp_dt, arp_ft, arp_enc): the 16-bit mode that meets north_star's 1e-4 / 1e-3; the train steps
                           carry an exact power-of-two scale on their backward activations (binary16's exponent range) */

#define ARP_MODE_F16X3 3 /* arp_enc only: f32-accurate products on the 16-bit MFMA -- every GEMM operand is an (hi, lo) pair of binary16 values and a
                           product is hi.hi + lo.hi + hi.lo (three MFMAs, ~2^-22 relative; a K-concatenated operand [x_hi | x_lo | x_hi] against
                           [W_hi | W_hi | W_lo] on the ordinary f16 kernels), attention / LayerNorm / residual stream in f32.  The 16-bit mode of row N1
                           that meets north_star's 1e-3 on the policy logits (the plain f16 encoder does not: DESIGN 6b) */
#define ARP_MODE_F16C 4  /* arp_enc only (round 5): the binary16 encoder with the operand ROUNDINGS of its GEMMs corrected on the scaled fp4 MFMA --
                           a product is x_hi.W_hi (binary16) + 2^-s x4.dW4 (+ 2^-s' dx4.W4) where dW = W - W_hi, dx = x - x_hi are carried as e2m1
                           (OCP fp4) with power-of-two block scales: the correction terms are 2^-12 of the product, 1-2 significant bits take the
                           roundings out to a quarter of their size, and the fp4 MFMA moves four times the k per cycle on the same 4-register operand
                           tuples, so a product with both corrections costs 1.5x the binary16 one instead of f16x3's 3x.  Patch embedding on (hi, lo)
                           binary16 pairs; attention, LayerNorm statistics, residual stream as in ARP_MODE_F16.  ARP_F16C_PLAN selects, per GEMM
                           (in_proj, out_proj, fc1, fc2), 0 = plain / 1 = weight correction / 2 = both */

#define ARP_ACT_NONE 0
#define ARP_ACT_QGELU 1
#define ARP_ACT_RELU 2
#define ARP_ACT_TANH 3
#define ARP_ACT_GELU_TANH 4

const char* arp_last_error(void);
int arp_version(void);
/* test hook: what the library's handles and entry points hold right now, process-wide: out5 = {device bytes, device buffers, streams, events, pinned host bytes}.
   Counts the library's own allocations only (not arp_dev_malloc / arp_event_create, which the caller frees). */
int arp_debug_live(int64_t out5[5]);
int arp_device_count(void); /* number of visible HIP devices; 0 when there is none (never fails) */

/* ---- raw device memory + events (for HBM-resident benchmarking; no torch types anywhere) ------ */
int arp_dev_malloc(void** out, size_t bytes);
int arp_dev_free(void* p);
int arp_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);
int arp_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);
int arp_set_device(int device);
/* Pin / unpin a caller-owned host buffer (hipHostRegister): host-fed calls then move it by true asynchronous DMA.  For buffers that are
   reused across calls (registration costs milliseconds per 100 MB); unregister before freeing the memory. */
int arp_host_register(void* p, size_t bytes);
int arp_host_unregister(void* p);
int arp_dev_synchronize(void); /* hipDeviceSynchronize on the current device */

/* ---- path (1): CLIP reward labelling ------------------------------------------------------------
 * Replaces clip.load(...) + the compute_reward closure, arp_dt/label_reward.py:125-146
 * (third-party openai/CLIP forward; in-tree mirror arp_dt/models/openai/layers.py:274-449). */
typedef struct arp_clip arp_clip;

typedef struct arp_clip_cfg {
    int32_t patch;      /* 32 (BASELINE headline) or 16 (what the reference loads, label_reward.py:126) */
    int32_t width;      /* 768 */
    int32_t layers;     /* 12  */
    int32_t heads;      /* 12  */
    int32_t embed;      /* 512 */
    int32_t img_res;    /* 224 */
    int32_t txt_width;  /* 512 */
    int32_t txt_layers; /* 12  */
    int32_t txt_heads;  /* 8   */
    int32_t ctx;        /* 77  */
    int32_t vocab;      /* 49408 */
    int32_t mode;       /* ARP_MODE_F32 | ARP_MODE_BF16 | ARP_MODE_F16 */
    int32_t device;     /* HIP device ordinal */
    int32_t max_batch;  /* frames per internal pass (workspace size); <= 0 -> 1024 */
    int32_t attn_impl;  /* 0 = auto (MFMA kernel where available), 1 = force the VALU kernel */
    int32_t n_streams;  /* N in 2..4 = label a batch in N contiguous parts (each >= 128 frames) on N HIP streams so one
                           part's memory-bound kernels and GEMM tails overlap another part's GEMMs; 0/1 = one stream */
} arp_clip_cfg;

int arp_clip_create(const arp_clip_cfg* cfg, arp_clip** out);
int arp_clip_destroy(arp_clip* h);

/* One tensor of an openai/CLIP state dict (names and layouts: arp_dt/models/openai/model.py:220-314,
 * SURVEY.md Appendix B), f32 host data, row-major.  Call arp_clip_finalize_weights() after the last. */
int arp_clip_load_weight(arp_clip* h, const char* name, const float* data, const int64_t* shape, int ndim);
/* Before arp_clip_finalize_weights: run the vision tower's c_fc / c_proj GEMMs on the scaled fp8 MFMA (e4m3 operands, f32 accumulate;
 * BASELINE.json configs[4] "bf16 with fp8 MFMA GEMMs").  A THROUGHPUT mode for the frozen towers of the fine-tune step
 * (finetune_module/clip_multiscale_adapter.py:134-175): 3 significand bits, features ~1e-2 off the f32 towers -- not for labelling
 * to 1e-4.  16-bit modes only, width % 128 == 0.  on = 2: the attention's in_proj / out_proj on fp8 operands as well, in blocks whose QKV +
 * attention do not run on the fused kernel (ViT-B/16's 197 tokens): ln_1 and the attention output are written as e4m3. */
int arp_clip_set_fp8_mlp(arp_clip* h, int on);
int arp_clip_finalize_weights(arp_clip* h);

/* clip.tokenize output [n_prompts, ctx] int32 -> runs the text tower ONCE and caches the normalised
 * text features (the reference re-runs it per trajectory, label_reward.py:136-141). */
int arp_clip_set_text(arp_clip* h, const int32_t* tokens, int n_prompts);
int arp_clip_get_text_features(arp_clip* h, float* out /* [n_prompts, embed], L2-normalised */);
/* Which reduction over the cached prompts a reward is: 0 (default) = logits_per_text[0], prompt 0 whatever was cached (the offline pass,
 * arp_dt/label_reward.py:146); 1 = logits_per_text.mean(axis=0) over all cached prompts -- the rollout loop's live branch for a LIST of prompts
 * (arp_dt/envs/vl_reward.py:19-22).  Applies to every labelling call of the handle until changed. */
int arp_clip_set_prompt_reduce(arp_clip* h, int mode);

/* compute_reward (label_reward.py:132-146): uint8 NHWC frames -> float32 rewards
 * = exp(logit_scale) * cos(image, prompt 0).  use_crop selects the transform of label_reward.py:92-102. */
int arp_clip_label(arp_clip* h, const uint8_t* frames_host, int n, int H, int W, int use_crop, float* rewards_host);
/* Same, frames and rewards already in device memory; enqueued on the handle's stream. */
/* Asynchronous form of arp_clip_label for a STREAM of calls (n <= max_batch each): submit() enqueues upload + pass + download on slot
 * 0 / 1 and returns, collect() waits for that slot.  Submitting call i+1 before collecting call i keeps the compute streams full across
 * calls (a synchronous call pays the pipeline's fill and drain every time).  `frames` must stay valid until collect() of the slot. */
int arp_clip_label_submit(arp_clip* h, int slot, const uint8_t* frames_host, int n, int H, int W, int use_crop);
int arp_clip_label_collect(arp_clip* h, int slot, float* rewards_host);
int arp_clip_label_dev_async(arp_clip* h, const uint8_t* frames_dev, int n, int H, int W, int use_crop,
                             float* rewards_dev);
int arp_clip_sync(arp_clip* h);
int arp_clip_set_streams(arp_clip* h, int n_streams); /* change the stream count, 0..4 (see arp_clip_cfg.n_streams) */

/* model.encode_image (label_reward.py:156, clip_goal_conditioned variant) */
int arp_clip_encode_image(arp_clip* h, const uint8_t* frames_host, int n, int H, int W, int use_crop, int normalize,
                          float* out /* [n, embed] */);
/* The same with frames and features in device memory: enqueued on the handle's stream (ordered against other streams by the caller's events), no copy out, no
 * wait.  At most max_batch frames per call; no prompt set needed.  The rollout session's goal reward (arp_rollout_create_gc) runs on it. */
int arp_clip_encode_image_dev_async(arp_clip* h, const uint8_t* frames_dev, int n, int H, int W, int use_crop, int normalize,
                                    float* feats_dev /* [n, embed] */);

/* The torchvision/PIL transform alone (label_reward.py:109-121 / :92-102), for PIL-parity tests:
 * uint8 NHWC -> f32 NCHW [n,3,res,res]. */
int arp_preprocess(const uint8_t* frames_host, int n, int H, int W, int use_crop, int res, float* out_nchw_host);
/* Host-side resample table (Pillow precompute_coeffs + normalize_coeffs_8bpc); no GPU needed.
 * xmin[out], cnt[out], weights[out*ksize_cap]; returns the max tap count or < 0. */
int arp_bicubic_coeffs(int in_size, int out_size, int32_t* xmin, int32_t* cnt, int32_t* weights, int ksize_cap);

/* Per-call-site HIP-event profile of the kernels launched on the handle's stream. */
int arp_clip_profile_enable(arp_clip* h, int on);
int arp_clip_profile_reset(arp_clip* h);
/* JSON object {"site": {"ms": total_ms, "calls": n}, ...}; returns bytes written or < 0. */
int arp_clip_profile_json(arp_clip* h, char* buf, int buf_len);

/* The shader clock the chip holds under the labelling pass (bench.py: whole_pass.clock_ghz).  on = 1 zeroes the accumulators and routes the vision
 * tower's c_fc launches through a DIAGNOSTIC instance of the same GEMM kernel that stamps s_memtime / s_memrealtime around every workgroup (the product
 * instances execute no stamp); rewards are unchanged.  arp_clip_clock_read: out[0] = GHz (sum of shader cycles / sum of 100 MHz ticks over the probed
 * workgroups), out[1] = workgroups probed, out[2] = mean workgroup duration in microseconds. */
int arp_clip_clock_probe(arp_clip* h, int on);
int arp_clip_clock_read(arp_clip* h, double* out3);

/* HIP events on the handle's stream (bench timing) */
typedef struct arp_event arp_event;
int arp_event_create(arp_event** out);
int arp_event_destroy(arp_event* e);
int arp_clip_event_record(arp_clip* h, arp_event* e);
int arp_event_elapsed_ms(arp_event* start, arp_event* stop, float* ms); /* synchronises on stop */

/* ---- path (2): ARP-DT policy train step ------------------------------------------------------------
 * Replaces create_train_step(...) -> train_step_fn(state, batch, rng), arp_dt/main_procgen.py:104-141
 * (model arp_dt/ARPDT.py:152-261,413-486 + arp_dt/layers.py; optimizer main_procgen.py:490-507).
 * Boundary: the frozen (stop_gradient) M3AE encodings are an input; adapter, image_text_input, token
 * embeddings, the causal transformer, both heads, losses, L2 term, gradient all-reduce, global-norm clip
 * and Adam are inside.  Tensors cross the boundary under their Flax tree path flattened with '/'
 * (e.g. "policy/Block_0/Attention_0/Dense_0/kernel"), in the Flax layout ([in, out] kernels). */
typedef struct arp_dt arp_dt;

typedef struct arp_dt_cfg {
    int32_t emb;         /* 128 */
    int32_t depth;       /* 2   */
    int32_t heads;       /* 8   */
    int32_t mlp_ratio;   /* 4   */
    int32_t n_actions;   /* 15  */
    int32_t window;      /* 4 time steps -> 12 tokens (8 for model BC) */
    int32_t enc_tokens;  /* 257 (M3AE ViT-B/16 at 256x256) */
    int32_t enc_dim;     /* 768 */
    int32_t use_adapter; /* 1   */
    int32_t mode;        /* ARP_MODE_F32 | ARP_MODE_F16 (default of arp_amd.train) | ARP_MODE_BF16: operand type of the adapter / image_text_input GEMMs */
    int32_t device;
    int32_t world;       /* data-parallel degree (set again by arp_dt_comm_init) */
    int32_t rank;
    float lambda_ret;    /* lambda_return_pred */
    float weight_decay;  /* coefficient of the explicit 0.5*wd*||p||^2 term (main_procgen.py:114-117) */
    float clip_norm;     /* optax.clip_by_global_norm */
    float b1, b2, eps;   /* adam */
    int32_t alibi_bias;  /* config.alibi_bias (arp_dt/layers.py:74-78; off in the shipped configuration): slope_h * key_index added to the policy
                            transformer's attention scores, slopes as _get_attention_slopes (layers.py:97-110) */
    int32_t model;       /* ARP_DT_MODEL_ARPDT (0, the default) | ARP_DT_MODEL_BC (1): the InstructRL baseline, arp_dt/BC.py (main_procgen.py:406-427
                            with use_vl=False, vl_type="BC") -- two tokens per time step [image, action], the action head on the image-token rows
                            0::2, no rtg_input, no return head, no return loss.  A BC handle takes rtg == NULL (and ignores a non-NULL one), wants
                            return_pred == NULL in arp_dt_forward, reports trans_loss = return_loss = 0 (the model outputs neither:
                            main_procgen.py:118-124,153-157 read them with output.get(..., 0.0)) and refuses arp_dt_attach_encoder.
                            ARP_DT_MODEL_GCBC (2): the goal-conditioned baseline, arp_dt/GCBC.py (main_procgen.py:413-414).  Its policy is BC's line for line
                            -- same parameter tree, same step, same aux; with encodings in, a GCBC and a BC handle give the same bits -- and what it
                            changes is the frozen encoder call: forward_gc_representations on a (frame, goal) pair (GCBC.py:462-468), which reads no
                            text.  So a GCBC handle ACCEPTS arp_dt_attach_encoder, with enc_tokens == 2 P + 1 (arp_enc_gc_tokens) and enc_dim == width,
                            and takes frames + goal frames through arp_dt_set_batch_images_goal. */
} arp_dt_cfg;
enum { ARP_DT_MODEL_ARPDT = 0, ARP_DT_MODEL_BC = 1, ARP_DT_MODEL_GCBC = 2 };

int arp_dt_create(const arp_dt_cfg* cfg, arp_dt** out);
int arp_dt_destroy(arp_dt* h);
int arp_dt_num_params(arp_dt* h, int64_t* total, int32_t* n_tensors);
int arp_dt_param_info(arp_dt* h, int i, char* name_buf, int name_len, int64_t* shape4, int32_t* ndim);
/* which: 0 = params, 1 = gradients (of the last backward), 2 = adam mu, 3 = adam nu */
int arp_dt_set_tensor(arp_dt* h, const char* name, int which, const float* data);
int arp_dt_get_tensor(arp_dt* h, const char* name, int which, float* out); /* which = 1 after a data-parallel step: the rank MEAN */
int arp_dt_set_step(arp_dt* h, int64_t step);
int arp_dt_get_step(arp_dt* h, int64_t* step);
/* Stages one per-device batch in HBM: enc f32 [B,T,enc_tokens,enc_dim], action int32 [B,T], rtg f32 [B,T,1] (NULL allowed for model BC). */
int arp_dt_set_batch(arp_dt* h, const float* enc, const int32_t* action, const float* rtg, int B);
/* ARPDT.__call__ on the staged batch: logits [B,T,n_actions], return_pred [B,T,1] (must be NULL for model BC, which has no return head),
 * metrics[4] = loss, acc (fraction), trans_loss, return_loss (any pointer may be NULL). */
int arp_dt_forward(arp_dt* h, float* action_logits, float* return_pred, float* metrics);
/* forward + backward + L2 term; gradients readable with arp_dt_get_tensor(.., 1, ..) (parity tests) */
int arp_dt_backward(arp_dt* h);
/* train_step_fn on the staged batch: forward, backward, L2 term, RCCL all-reduce (when a communicator is
 * attached), clip_by_global_norm, adam.  aux[9] = loss, acc*100, trans_loss, return_loss, weight_penalty,
 * weight_l2, train_state_step, learning_rate, (extra) gradient norm. */
int arp_dt_train_step(arp_dt* h, float lr, float* aux);
int arp_dt_train_step_async(arp_dt* h, float lr); /* no read-back; pair with arp_dt_sync */
/* val_step_fn of create_val_step (main_procgen.py:144-169): forward on the staged batch, rank mean (pmean, :165) of
   aux4 = {loss, trans_loss, return_loss, acc * 100}.  No parameter changes. */
int arp_dt_val_step(arp_dt* h, float* aux4);
/* Two device-resident batch slots (0 / 1) = prefetch_to_device(..., 2) of main_procgen.py:703.  upload_*_async copies a host batch
   into a slot on the handle's copy stream and returns without waiting for the GPU; it touches only that slot, so a prefetch thread
   may call it while arp_dt_train_step runs on the other slot (the copy itself waits, on the GPU, for the last step that read the
   slot).  select_batch makes the next forward / val_step / train_step read a slot, ordered behind its upload.  arp_dt_set_batch
   (synchronous) keeps writing the selected slot.  Pinned host memory makes the copy truly asynchronous; pageable works (staged). */
int arp_dt_upload_batch_async(arp_dt* h, int slot, const float* enc, const int32_t* action, const float* rtg, int B);
int arp_dt_upload_batch_images_async(arp_dt* h, int slot, const float* images, const int32_t* action, const float* rtg, int B);
int arp_dt_select_batch(arp_dt* h, int slot);
/* The data-parallel step all-reduces the flat gradient in two buckets of two ranges each; bucket 1 (image_text_input's kernel and
   everything the transformer owns) is launched on a communication stream while the adapter's backward GEMMs still run.
   ranges8 = {lo, hi} x 4 in floats (bucket 1: ranges 0, 1; bucket 2: ranges 2, 3), *total = the flat parameter count.  Needs no GPU.
   Environment: ARP_DT_OVERLAP=0 selects the serial form (one all-reduce behind the whole backward), ARP_DT_FORCE_COMM=1 runs the
   all-reduce path at world = 1 as well. */
int arp_dt_bucket_plan(const arp_dt_cfg* cfg, int64_t* ranges8, int64_t* total);
int arp_dt_sync(arp_dt* h);
int arp_dt_event_record(arp_dt* h, arp_event* e);
/* Data parallelism: one process per GPU.  Rank 0 calls arp_dt_comm_unique_id, ships the 128 bytes to the
 * others (any side channel), every rank calls arp_dt_comm_init, then arp_dt_broadcast_state
 * (= sync_state_fn, main_procgen.py:94-101). */
int arp_dt_comm_unique_id(void* id128);
int arp_dt_comm_init(arp_dt* h, const void* id128, int world, int rank);
int arp_dt_broadcast_state(arp_dt* h);
/* ARP_MODE_F16 only: the adapter's two FORWARD products (models/adapter/layers.py:19-30) with their binary16 operand roundings corrected on the scaled fp4 MFMA
 * (ARP_MODE_F16C's product) and the adapter output handed to the residual mix inside image_text_input's operand load (binary16 + the e2m1 code of its
 * rounding error; ARP_DT_ADAPTER_PLAN): takes the policy's own share out of the encoder-inside logit error (row N1) for ~0.1 ms per step.  On by default in
 * f16 where enc_dim is a multiple of 256 and >= 512 (ARP_DT_ADAPTER_C=0 turns it off at create); the backward is unchanged.  May be called at any time:
 * the next calls run eagerly and capture the step's chain again. */
int arp_dt_set_adapter_corrections(arp_dt* h, int on);
/* test hook: the bytes of a named intermediate device buffer of the last forward ("Xc", "H1c", "W1c", "W2c", "wc_scal", "A32", "A", "Adx", "Y", "img", "H1", "Xb");
   copies min(bytes, size), returns the buffer's size or -1 */
int64_t arp_dt_debug_read(arp_dt* h, const char* name, void* out, int64_t bytes);
/* What the communicator says about itself, for a multi-GPU run that certifies itself (the pmean of main_procgen.py:132 needs every
 * device in it): info5 = {ncclCommCount, ncclCommUserRank, ncclCommCuDevice, ncclGetVersion code, 1 if a communicator exists};
 * without one (world 1) {1, 0, device, 0, 0}.  arp_dt_comm_selfcheck all-reduces (sum) the scalar rank + 1 through that
 * communicator on the step's stream: every rank must read world (world + 1) / 2 (without a communicator: 1, nothing reduced). */
int arp_dt_comm_info(arp_dt* h, int32_t* info5);
int arp_dt_comm_selfcheck(arp_dt* h, double* sum);
int arp_dt_profile_enable(arp_dt* h, int on);
int arp_dt_profile_reset(arp_dt* h);
int arp_dt_profile_json(arp_dt* h, char* buf, int buf_len);

/* ---- row N2: CLIP multi-scale adapter fine-tune step (BASELINE.json configs[4]) --------------------------------
 * The trainable head of finetune_module/clip_multiscale_adapter.py::CLIPMultiscaleAdapter on top of the FROZEN CLIP
 * towers (finetune_module/finetune.py:139-140): encode_image :134-149, encode_text :151-175, forward :177-250
 * (VIP loss + lambda_id * inverse-dynamics CE), optimiser torch.optim.AdamW over every non-CLIP parameter (:141).
 * The towers' outputs are the step's inputs: the per-block CLS (image) / EOT (text) features the reference collects with
 * forward hooks (finetune_module/utils.py:6-18), concatenated block 0..layers-1, and the final CLIP features.
 * Parameters cross under torch's state_dict names with torch's [out, in] Linear layout:
 *   "image_intermediate_linear.weight", "text_intermediate_linear.weight", "{image,text}_adapter.layers.{0,3}.{weight,bias}",
 *   "inverse_layer.layers.{0,3}.{weight,bias}", "image_residual_weight", "text_residual_weight", "lambda_id". */
typedef struct arp_ft arp_ft;
typedef struct arp_ft_cfg {
    int32_t layers;     /* clip_model.transformer.layers (12): blocks whose features are concatenated, both towers */
    int32_t width_v;    /* 768 */
    int32_t width_t;    /* 512 (= input_dim = output_dim of the reference constructor) */
    int32_t embed;      /* 512 */
    int32_t hidden;     /* hidden_dim 1024: adapters use hidden*(layers+1), the inverse model uses hidden */
    int32_t n_actions;  /* 15 */
    int32_t mode;       /* ARP_MODE_F32 | ARP_MODE_F16 (default of arp_amd.finetune) | ARP_MODE_BF16 */
    int32_t device;
    int32_t use_vip;    /* use_vip_loss */
    int32_t use_id;     /* use_id_loss */
    float gamma;        /* 0.98 (:107) */
    float logit_scale;  /* ln of the similarity scale, clip_model.logit_scale (:95) */
    float weight_decay; /* AdamW decoupled decay, finetune.py:31 (0.001) */
    float b1, b2, eps;  /* 0.9, 0.999, 1e-8 */
    int32_t goal_conditioned; /* clip_multiscale_adapter.py:208-212,224-230: the batch carries FOUR image groups (image0..image3); image3's
                                 adapted feature takes the prompt's place -- scores = -||a3 - a_k||, inverse-model input [a1|a3|a2|a3] --
                                 and the text head is never run (its parameters get no gradient and AdamW leaves them alone) */
} arp_ft_cfg;
/* The frozen towers' side of the step, on an arp_clip handle (ViT-B/16 in the reference, :118): per-block CLS / EOT
 * features and the un-normalised CLIP features.  Image frames go through the fine-tune transform of :120-132 (float,
 * bilinear resize to 224 when both sides differ, /255, normalise) -- NOT the PIL-bicubic one of label_reward.py; the
 * random ColorJitter of training (:24-36) belongs to the data pipeline and is not applied. */
int arp_clip_encode_image_multiscale(arp_clip* h, const uint8_t* frames_nhwc, int n, int H, int W,
                                     float* inter /* [n, layers*width] */, float* final_feat /* [n, embed] */);
int arp_clip_encode_text_multiscale(arp_clip* h, const int32_t* tokens /* [n, ctx] */, int n,
                                    float* inter /* [n, txt_layers*txt_width] */, float* final_feat /* [n, embed] */);
/* The same two calls with their OUTPUTS in device memory (arp_dev_malloc), for arp_ft_set_batch_dev: the tower features
 * then never cross PCIe. */
int arp_clip_encode_image_multiscale_dev(arp_clip* h, const uint8_t* frames_nhwc, int n, int H, int W, float* inter_dev, float* final_dev);
/* The same two outputs through the LABEL transform (Pillow-exact bicubic resize + normalise, use_crop as in arp_clip_label) instead of the
 * fine-tune transform: what the rollout loop's adapter rewards hand the fine-tuned model -- `model.encode_image(preprocess(Image.fromarray(obs)))`,
 * arp_dt/envs/vl_reward.py:44-61 (get_torch_clip_adapter_reward) and :64-79 (..._goal_conditioned_reward).  A call of a few frames runs on the
 * latency path. */
int arp_clip_encode_image_multiscale_pil(arp_clip* h, const uint8_t* frames, int n, int H, int W, int use_crop, float* inter, float* final_feat);
int arp_clip_encode_text_multiscale_dev(arp_clip* h, const int32_t* tokens, int n, float* inter_dev, float* final_dev);
int arp_ft_create(const arp_ft_cfg* cfg, arp_ft** out);
int arp_ft_destroy(arp_ft* h);
int arp_ft_num_params(arp_ft* h, int64_t* total, int32_t* n_tensors);
int arp_ft_param_info(arp_ft* h, int i, char* name_buf, int name_len, int64_t* shape4, int32_t* ndim);
/* which: 0 = parameter, 1 = gradient, 2 = AdamW exp_avg, 3 = AdamW exp_avg_sq.  Gradients: arp_ft_backward stores every one; a single-process
 * arp_ft_train_step applies the seven big weight gradients inside their GEMMs and never stores them -- reading one of those afterwards is an error
 * (ARP_FT_FUSE_ADAM=0 restores the stored gradients and the separate AdamW pass). */
int arp_ft_set_tensor(arp_ft* h, const char* name, int which, const float* data);
int arp_ft_get_tensor(arp_ft* h, const char* name, int which, float* out);
/* f16 mode only: gradient elements that arrived at AdamW as inf / NaN (a binary16 overflow in the x 1024-seeded backward) and were treated
   as missing for that step -- cumulative since create.  The other modes never mask: a non-finite gradient shows as NaN parameters, as in
   torch.optim.AdamW (finetune_module/finetune.py:141). */
int arp_ft_dropped_gradients(arp_ft* h, uint64_t* count);
int arp_ft_set_step(arp_ft* h, int64_t step);
int arp_ft_get_step(arp_ft* h, int64_t* step);
/* img_inter [3, B, layers*width_v] and img_final [3, B, embed]: frames image0, image1, image2 of each sample
 * (clip_multiscale_adapter.py:185-202; image3 is only read when goal_conditioned); txt_inter [B, layers*width_t],
 * txt_final [B, embed]; r [B] as stored in the batch (the loss uses r - 1, :215); action [B] class ids. */
int arp_ft_set_batch(arp_ft* h, const float* img_inter, const float* img_final, const float* txt_inter, const float* txt_final,
                     const float* r, const int32_t* action, int B);
int arp_ft_set_batch_dev(arp_ft* h, const float* img_inter_dev, const float* img_final_dev, const float* txt_inter_dev,
                         const float* txt_final_dev, const float* r /* host */, const int32_t* action /* host */, int B);
/* metrics4: loss, vip_loss, id_loss, lambda_id.  scores [3, B] and logits [B, n_actions] may be NULL. */
int arp_ft_forward(arp_ft* h, float* metrics4, float* scores, float* logits);
/* Inference half of one tower's head -- model.encode_image (which = 0) / model.encode_text (which = 1) as the clip_ft
 * labelling branch calls them (arp_dt/label_reward.py:165-230): tower features [n, layers*width] + [n, embed] -> adapted,
 * L2-normalised features [n, layers*width_t + embed].  Drops a batch staged with arp_ft_set_batch. */
int arp_ft_encode(arp_ft* h, int which, const float* inter, const float* final_feat, int n, float* out);
/* ---- the fine-tuned CLIP reward, resident on the device (model_type = "clip_ft": label_reward.py:165-230, envs/vl_reward.py:44-61) ----
 * uint8 frames in HBM -> frozen towers (`towers`: a finalized arp_clip on the same device whose widths, layers and embed are the head's) -> the head's
 * inference pass -> exp(logit_scale) <adapted image, adapted prompt> as one f32 per frame in HBM.  Everything is enqueued on the TOWERS' stream; the only
 * synchronisations are the ones named below.  The pass has a workspace of its own: a batch staged with arp_ft_set_batch survives it.  It rounds where the
 * training forward rounds (tower features, [U | final] and the hidden layer become the operand type; the rest is f32).
 * arp_ft_reward_set_text: the text side, once per prompt set, cached on the device (adapted, normalised prompts and their mean); synchronises.  The cache
 * belongs to the parameters of that moment: after arp_ft_set_tensor(which = 0), a train step or arp_ft_broadcast_state every reward call is REFUSED until
 * the text is set again.  transform: 0 = the fine-tune transform (bilinear; use_crop = the centre crop of side W / 2 at int((H - cs) / 2), int((W - cs) / 2),
 * taken on the device: label_reward.py:200-230), 1 = the label transform (Pillow bicubic, use_crop as arp_clip_label: envs/vl_reward.py:44-61).
 * arp_ft_reward_dev_async: any n >= 1, chunks of the towers' max_batch in stream order, no synchronisation; a call that fits the towers' latency path is
 * captured once per (buffers, n, geometry, transform, reduction) and replayed (ARP_FT_REWARD_GRAPH=0: launch by launch).  arp_ft_reward: the same from
 * and to host memory (pinned staging while a chunk is at most 8 MiB of frames), one synchronisation per chunk; writes rewards[0 .. n - 1] only.
 * Refused with a message: towers and head on different devices or of different geometry, a goal_conditioned head, no prompts cached, stale prompts, null
 * or empty buffers.  The two handles stay the caller's; the towers' stream must not be used by another host thread during a call. */
int arp_ft_reward_set_text(arp_ft* h, arp_clip* towers, const int32_t* tokens /* [n_prompts, ctx] */, int n_prompts);
int arp_ft_reward_set_reduce(arp_ft* h, int mean); /* 0: prompt 0 (label_reward.py:228), 1: the mean over the prompts (:226, envs/vl_reward.py:56-57) */
int arp_ft_reward_dev_async(arp_ft* h, arp_clip* towers, const uint8_t* frames_dev, int n, int H, int W, int use_crop, int transform, float* rewards_dev);
int arp_ft_reward(arp_ft* h, arp_clip* towers, const uint8_t* frames, int n, int H, int W, int use_crop, int transform, float* rewards);
/* The reward kernel of that path alone: reward[r] = scale * <y, t> / max(||y||, 1e-12), y = s f[r] + (1 - s) A[r], s = sigmoid(rw); t = prompt row 0, or
 * (mean = 1) the mean of the n_prompts rows [n_prompts, F], taken on the device.  f, A [rows, F]; all f32 host arrays. */
/* Calls of at most 16 rows run the head's three products on a weight-streaming kernel (csrc/ftrows.h; 16-bit modes) unless on = 0 (or ARP_FT_ROWS=0):
 * then, as for more rows, the training GEMMs.  arp_ft_reward_stats: out4 = {captured chains replayed, chains captured, calls launched one by one,
 * products run on the rows kernel} since the handle was created.
 * Ordering against training: the reward calls run on the TOWERS' stream and read the head's parameters.  Every reward call records an event behind
 * itself; arp_ft_set_tensor of a parameter, the train steps and arp_ft_broadcast_state wait for it before the parameters move, and the version rule
 * refuses the reward calls made after that. */
int arp_ft_reward_set_rows(arp_ft* h, int on);
int arp_ft_reward_stats(arp_ft* h, int64_t out4[4]);
/* The rows kernel alone + the split-K reduce behind it: out[m, n] (ldo; out_rows >= M rows prefilled by the caller, only [0, M) x [0, N) is written) =
 * act(A[M, K] (lda) . W[N, K]^T (ldw) + bias), operands in the type of `mode` (bf16 / f16), output in that type (widened back) or f32.  act: none or relu.
 * ksplit = 0: the dispatcher's slice count.  Returns the slice count used; -1 with a message outside the domain (1 <= M <= 16, K % 64 == 0, N % 16 == 0,
 * lda and ldw multiples of 8) -- nothing is written then. */
int arp_op_ft_rows_gemm(int mode, int act, const float* A, int lda, const float* W, int ldw, const float* bias, float* out, int ldo, int out_rows, int out_f32,
                        int M, int N, int K, int ksplit);
int arp_op_ft_reward(const float* f, const float* A, float rw, const float* t, int n_prompts, int mean, float scale, float* reward, int rows, int F);
int arp_ft_backward(arp_ft* h);                        /* forward + backward: fills every gradient */
int arp_ft_train_step(arp_ft* h, float lr, float* aux4); /* forward + backward + AdamW; aux4 as metrics4 (pre-update) */
int arp_ft_train_step_async(arp_ft* h, float lr);
int arp_ft_sync(arp_ft* h);
int arp_ft_event_record(arp_ft* h, arp_event* e);
/* Data parallelism for the head step (BASELINE.json configs[4]: DP = 8; the reference's finetune.py is single-GPU): one process
 * per GPU, id from arp_dt_comm_unique_id on rank 0, then every step all-reduces the flat f32 gradient once (sum; the mean is
 * folded into the AdamW kernel) -- the scheme of the policy step (main_procgen.py:128-139). */
int arp_ft_comm_init(arp_ft* h, const void* id128, int world, int rank);
int arp_ft_broadcast_state(arp_ft* h);
int arp_ft_comm_info(arp_ft* h, int32_t* info5);       /* as arp_dt_comm_info / arp_dt_comm_selfcheck, on the head step's communicator */
int arp_ft_comm_selfcheck(arp_ft* h, double* sum);
/* The data-parallel step all-reduces the 1.9 GB gradient in seven buckets in the order the backward produces them (inverse model;
   per tower: second adapter layer, first adapter layer, intermediate linear), each launched on a communication stream as soon as its
   last weight-gradient GEMM is enqueued.  ranges28 = {lo, hi} x 14 in floats (bucket b = ranges 2b, 2b + 1; empty ranges have
   lo = hi), *total = the flat parameter count.  Needs no GPU.  ARP_FT_OVERLAP=0: one all-reduce behind the whole backward;
   ARP_FT_FORCE_COMM=1: the all-reduce path at world = 1 too.  arp_ft_get_tensor(which = 1) after such a step: the rank MEAN. */
int arp_ft_bucket_plan(const arp_ft_cfg* cfg, int64_t* ranges28, int64_t* total);
int arp_ft_profile_enable(arp_ft* h, int on);
int arp_ft_profile_reset(arp_ft* h);
int arp_ft_profile_json(arp_ft* h, char* buf, int buf_len);

/* ---- row N1: frozen M3AE image encoder (forward_representation) -----------------------------------
 * arp_dt/models/m3ae/model.py:471-496 as called under stop_gradient by arp_dt/ARPDT.py:413-462.
 * Weights cross under their Flax tree path ('/'-flattened, [in,out] kernels): "cls_token",
 * "encoder_image_type_embedding", "image_embedding/{kernel,bias}", "encoder/Block_i/...", "encoder/LayerNorm_0/...". */
typedef struct arp_enc arp_enc;
typedef struct arp_enc_cfg {
    int32_t patch;      /* 16  */
    int32_t width;      /* 768 */
    int32_t layers;     /* 12  */
    int32_t heads;      /* 12  */
    int32_t mlp_ratio;  /* 4   */
    int32_t img_res;    /* 256 -> 257 tokens */
    int32_t mode;       /* ARP_MODE_F32 | ARP_MODE_F16 | ARP_MODE_BF16 | ARP_MODE_F16X3 | ARP_MODE_F16C (need not equal the mode of the policy handle it is attached to) */
    int32_t device;
    int32_t max_frames; /* frames per internal pass; <= 0 -> 128 */
    int32_t attn_impl;  /* 0 auto, 1 VALU */
} arp_enc_cfg;
int arp_enc_create(const arp_enc_cfg* cfg, arp_enc** out);
int arp_enc_destroy(arp_enc* h);
int arp_enc_load_weight(arp_enc* h, const char* name, const float* data, const int64_t* shape, int ndim);
int arp_enc_finalize_weights(arp_enc* h);
/* images f32 NHWC [n,res,res,3] (already normalised, as the training pipeline delivers them) -> f32 [n,tokens,width] */
int arp_enc_forward(arp_enc* h, const float* images_host, int n, float* out_host);
/* The goal-conditioned call (forward_gc_representations, arp_dt/models/m3ae/model.py:498-525; GCBC's encoder call, arp_dt/GCBC.py:462-468): n (frame, goal)
 * pairs, both f32 NHWC [n,res,res,3] -> f32 [n, 2 P + 1, width] with P = (img_res / patch)^2.  One sequence per pair: class token, the frame's P patches, the goal
 * frame's P patches; both patch blocks carry the same 2-D sincos position and image type embedding.  Both frame sets share one patch-embedding product; at
 * 256 x 256 the blocks run over 513 tokens, on the key-blocked attention kernels (csrc/attention_long.h).  max_frames counts pairs in this call; part streams
 * apply as in arp_enc_forward, and so does the latency path (arp_enc_set_latency: off for this call unless host_calls = 1; counted on n (2 P + 1) rows).  Modes f32, f16, bf16, f16x3; ARP_MODE_F16C returns an error (its attention output form
 * exists up to 288 tokens only).  arp_enc_gc_tokens: 2 P + 1. */
int arp_enc_forward_gc(arp_enc* h, const float* images_host, const float* goals_host, int n, float* out_host);
int arp_enc_gc_tokens(arp_enc* h);
/* The image + text call (forward_representation(image, text, text_padding_mask), arp_dt/models/m3ae/model.py:471-496; InstructRL's encoder call, arp_dt/BC.py:283-321):
 * n frames f32 NHWC [n,res,res,3] and an instruction of L token ids -> f32 [n, 1 + P + L, width].  One sequence per frame: class token, the frame's P patches, then
 * row 1 + P + i = text_embedding[tokens[i]] + get_1d_sincos_pos_embed(width, L)[i] + encoder_text_type_embedding.  mask f32, > 0 = padded (the reference's
 * convention): a padded text key is taken out of every softmax (model.py:247-250) -- as one bit per key for the key-masked attention kernels
 * (csrc/attention_long.h), which every text call runs on whatever its length; class and patch keys are always visible.  tokens (int32) and mask are [L], shared by
 * the n frames (per_row = 0), or [n, L] (per_row = 1).  Needs the optional weights "text_embedding/embedding" [vocab, width] and "encoder_text_type_embedding"
 * [1,1,width] (arp_enc_load_weight; vocab = the loaded tensor's first dimension) -- without both the call returns an error, and with them the other two calls are
 * unchanged bit for bit.  Ids outside [0, vocab) are refused.  1 + P + L <= 1024, head_dim 64.  Modes f32, f16, bf16, f16x3 (the exact-f32 masked attention + the
 * split pass); ARP_MODE_F16C returns an error.  max_frames, the part streams and the latency path apply as in arp_enc_forward, the latter on n (1 + P + L) rows.
 * arp_enc_text_tokens: 1 + P + L. */
int arp_enc_forward_text(arp_enc* h, const float* images_host, int n, const int32_t* tokens, const float* mask, int L, int per_row, float* out_host);
int arp_enc_text_tokens(arp_enc* h, int L);
/* Part streams (round 6): a call's frames are encoded as `n_streams` contiguous parts (1..4, default 2), part 0 on the caller's stream and the others on
 * streams of their own, so that one part's memory-bound kernels and GEMM grid tails run beside another part's GEMMs -- as arp_clip_cfg.n_streams does
 * for the labelling pass.  first_part_frames > 0: that many frames in part 0 of two; 0: the default cut (15/32 of the frames: parts that end at different times
 * fill each other's grid tails better, -1.5 % per step); < 0: equal parts.  A part of fewer than min_part_frames frames (<= 0: keep the default, 24) is not cut off.  Encodings are bit-identical for every setting. */
int arp_enc_set_streams(arp_enc* h, int n_streams, int first_part_frames, int min_part_frames);
/* Latency path: a call of at most `rows` token rows in total (frames x tokens; default 514: two frames at 257 tokens, beyond which the path
 * measured slower; capped at 1024), in ARP_MODE_F16 / ARP_MODE_BF16,
 * runs the W-tiled skinny GEMMs with split-K out_proj / c_proj whose reduction applies the next LayerNorm (csrc/tower.h::run_blocks) instead of the throughput
 * tiles: same operands, same accumulation type, another summation order.  Only a rollout session's per-step pass takes it by default; host_calls = 1 makes
 * arp_enc_forward and arp_enc_forward_gc take it too (0: not; < 0: unchanged); a goal-conditioned call counts pairs x (2 P + 1) rows.  rows = 0 turns the path off for every caller.  The training paths never take it.
 * Environment: ARP_ENC_LAT_ROWS sets `rows` at create. */
int arp_enc_set_latency(arp_enc* h, int rows, int host_calls);
int arp_enc_profile_enable(arp_enc* h, int on);
int arp_enc_profile_json(arp_enc* h, char* buf, int buf_len);
/* Put the frozen encoder INSIDE the policy step: after attaching, arp_dt_set_batch_images stages raw frames
 * [B,T,res,res,3] f32 and every forward / train step runs the encoder first (on the step's stream). */
int arp_dt_attach_encoder(arp_dt* h, arp_enc* enc);
/* InstructRL (model BC) with frames in: attach the encoder for its image + text pass (arp_enc_forward_text) together with ONE instruction, the instruction of
 * the game being trained -- tokens int32 [L], mask f32 [L] (> 0 = padded).  (BC.encode, arp_dt/BC.py:290-291, tiles the batch's instructions with
 * jnp.tile(text, (T, 1)), which pairs frame row i with instruction i mod B, not i // T: the reference is only meaningful with one instruction per batch.)
 * A BC handle only (arp_dt_attach_encoder keeps refusing it; ARP-DT and GCBC handles are refused here); enc_tokens == 1 + P + L (arp_enc_text_tokens) and
 * enc_dim == width; the encoder must carry the text weights.  Afterwards every frames slot of the handle encodes with the text pass: arp_dt_set_batch_images (rtg
 * NULL), arp_dt_upload_batch_images_async, arp_dt_encode_ahead, and index batches of frames from a device-resident set -- the same stager, slots and protocol as
 * the other two models.  The handle owns its copy of the instruction. */
int arp_dt_attach_text_encoder(arp_dt* h, arp_enc* enc, const int32_t* tokens, const float* mask, int L);
int arp_dt_set_batch_images(arp_dt* h, const float* images, const int32_t* action, const float* rtg, int B);
/* Model GCBC's staging slot (synchronous, like arp_dt_set_batch_images): frames and goal frames, both [B,T,res,res,3] f32, and the actions; every forward /
 * train step then runs the goal-conditioned encoder pass (arp_enc_forward_gc's) first.  The goal row is drawn per sample (data_procgen.py:186-189), so the
 * encoding depends on the pair and cannot come from a per-frame cache: for this model the encoder is inside the step.  The feed that keeps frames off PCIe
 * is the device-resident set's: arp_dt_set_batch_index_pairs / arp_dt_upload_batch_index_pairs_async (below) gather frames and goal frames into any slot, and
 * arp_dt_encode_ahead accepts slots 0 / 1 of a GCBC handle once they hold such a batch.  Not offered, each with an error string: HOST-built goal batches in
 * the two prefetch slots (arp_dt_upload_batch_images_async), arp_dt_encode_ahead on the synchronous slot (its step encodes it), a plain index batch
 * (arp_dt_*_batch_indices: it names no goal rows), a GCBC encodings cache, and arp_dt_set_batch_images (no goals) on a GCBC handle. */
int arp_dt_set_batch_images_goal(arp_dt* h, const float* images, const float* goals, const int32_t* action, int B);
/* The encoder is frozen: batch i + 1's encodings depend on nothing step i computes.  arp_dt_encode_ahead(slot) enqueues the encoder pass of the frames in
 * batch slot `slot` (0 / 1: uploaded with arp_dt_upload_batch_images_async; 2: staged by arp_dt_set_batch_images) on the encoder's own stream NOW -- behind the
 * slot's upload and the last step that read the slot -- so that it runs beside the current step's policy part; the step that then reads the slot waits for it
 * instead of encoding.  Callable from the uploader thread.  Without it a step encodes its own batch at its head (same stream of work, same encodings).
 * Model GCBC: slots 0 / 1 once arp_dt_upload_batch_index_pairs_async has filled them (the goal-conditioned pass); slot 2 is refused, its step encodes it. */
int arp_dt_encode_ahead(arp_dt* h, int slot);

/* ---- a demonstration set resident in HBM: policy batches from row indices -------------------------
 * ProcgenDataset.__getitem__ (arp_dt/data_procgen.py:180-213) reads ob[i][-T:] of a file whose rows the recorder stacks (row i adds one frame, ob[i, -1]).
 * The handle keeps that one uint8 frame per row [n_rows, res, res, 3], per-row action / return-to-go / first row of the trajectory, and optionally one
 * encoding per row; position t of the window of row i reads row j = max(i - (T - 1 - t), traj_start[i]).  res * res * 3 must be a multiple of 16. */
typedef struct arp_ds arp_ds;
int arp_ds_create(int64_t n_rows, int res, int device, arp_ds** out);
int arp_ds_destroy(arp_ds* ds);
int arp_ds_upload_frames(arp_ds* ds, int64_t row0, int64_t n, const uint8_t* u8_host); /* rows [row0, row0 + n), synchronous: callable chunk by chunk */
/* rtg may be NULL (model BC reads none).  Checked here, once: actions in [0, n_actions), 0 <= traj_start[i] <= i, traj_start non-decreasing. */
int arp_ds_set_labels(arp_ds* ds, const int32_t* action, const float* rtg, const int32_t* traj_start, int n_actions);
/* lut[c * 256 + u]: the f32 value of byte u in channel c.  A gathered frame holds exactly these values. */
int arp_ds_set_lut(arp_ds* ds, const float* lut768);
int arp_ds_alloc_encodings(arp_ds* ds, int tokens, int dim); /* tokens * dim a multiple of 4 */
int arp_ds_upload_encodings(arp_ds* ds, int64_t row0, int64_t n, const float* f32_host);
/* Every frame through `enc` into the encoding cache, `chunk` rows at a time (<= 0: 128).  Synchronous.  Must not run beside a prefetcher or a step of a policy
 * handle `enc` is attached to (they share the encoder's workspace). */
int arp_ds_encode(arp_ds* ds, arp_enc* enc, int chunk);
/* Debug read-back of the batch the indices name: f32 [B, window, res, res, 3], int32 [B, window], f32 [B, window]; each output may be NULL. */
int arp_ds_gather_debug(arp_ds* ds, const int64_t* idx, int B, int window, float* frames_out, int32_t* action_out, float* rtg_out);
int64_t arp_ds_nbytes(arp_ds* ds); /* HBM the handle holds */
/* A batch named by B row indices into slot 0 / 1 (asynchronous, the protocol of arp_dt_upload_batch_async) or the synchronous slot: gather kernels on the handle's
 * copy stream write the slot's frames (use_encodings == 0: needs an attached encoder of the dataset's res) or its encodings (use_encodings != 0: needs the cache,
 * [enc_tokens, enc_dim] per row) and its labels.  Every index and every geometry is checked on the host first; idx need not outlive the call. */
int arp_dt_upload_batch_indices_async(arp_dt* h, int slot, arp_ds* ds, const int64_t* idx, int B, int use_encodings);
int arp_dt_set_batch_indices(arp_dt* h, arp_ds* ds, const int64_t* idx, int B, int use_encodings);
/* Model GCBC: B (row, goal row) pairs.  The goal frames of sample b are the window of row goal_idx[b] under the same rule (data_procgen.py:189: ob[g][-T:]);
 * ONE frame-gather launch (grid z = 0 / 1) fills the slot's frames and goal frames, the actions follow idx, no return-to-go is read.  Same slots, copy stream
 * and protocol as the two calls above.  Checked on the host before anything is enqueued: everything arp_dt_set_batch_indices checks for frames, every
 * goal_idx[b] in [0, n_rows) (bounds only, not the hindsight rule: evaluation names goals from elsewhere), model GCBC, an attached encoder. */
int arp_dt_upload_batch_index_pairs_async(arp_dt* h, int slot, arp_ds* ds, const int64_t* idx, const int64_t* goal_idx, int B);
int arp_dt_set_batch_index_pairs(arp_dt* h, arp_ds* ds, const int64_t* idx, const int64_t* goal_idx, int B);
/* Debug read-back of a pair batch: frames_out and goals_out f32 [B, window, res, res, 3], action_out int32 [B, window]; each output may be NULL. */
int arp_ds_gather_pairs_debug(arp_ds* ds, const int64_t* idx, const int64_t* goal_idx, int B, int window, float* frames_out, float* goals_out, int32_t* action_out);
/* The fine-tune step's quads.  arp_ds_set_quad_bounds: first / last int32 [n_rows], the trajectory interval each row's four frames are taken from
 * (ProcgenActionDataset.bounds()); 0 <= first <= last < n_rows is checked for every row, first <= row <= last is NOT (the rows behind the last done flag
 * carry trajectory 0's interval: the reference's quirk).  Sample i reads q = sort(first[i], i, min(i + 1, last[i]), last[i]); r = q[2] == q[3]; its action
 * is action[q[0]].  arp_ds_quads_debug: read-back of the quad kernel for B indices and G = 3 / 4 groups -- rows_out int32 [G, B] (group-major), r_out f32 [B],
 * action_out int32 [B]; the same host checks as a staging; a store past the end of an output is detected on the device and is an error. */
int arp_ds_set_quad_bounds(arp_ds* ds, const int32_t* first, const int32_t* last);
int arp_ds_quads_debug(arp_ds* ds, const int64_t* idx, int B, int G, int32_t* rows_out, float* r_out, int32_t* action_out);
/* The feed: fine-tune batches built on the device from a resident demonstration set (finetune_module/action_finetune_data_procgen.py's four frames per
 * sample).  A batch is B row indices of `ds` (processed indices: file rows), which needs its frames, labels and quad bounds (arp_ds_set_quad_bounds).
 * arp_ft_feed_attach checks device and geometry, runs the text tower's multi-scale export once for the ONE prompt every sample shares (tokens [1, ctx]; NULL
 * for -- and only for -- a goal_conditioned head) and keeps it in HBM; the two slots' buffers come with the first staging of a size.  Everything belongs to
 * the head handle (arp_debug_live counts it); arp_ft_feed_detach and arp_ft_destroy give it back.  towers and ds must outlive the attachment.
 * arp_ft_feed_stage_async(slot 0 / 1): on the HOST first -- labels, quad bounds and every frame row present, every idx in [0, n_rows), the set's actions fit
 * the head, groups * B <= the towers' max_batch (groups = 3, or 4 for a goal_conditioned head) -- then on the TOWERS' stream: index upload, wait for the
 * slot's `consumed` event, the quad kernel, the fine-tune transform reading the resident frames through the row table + the vision tower for groups * B
 * frames, the export copied into the slot, the slot's `ready` event.  No host synchronisation.
 * arp_ft_feed_train_step_async: the head's stream waits for `ready`, copies the slot into the step's inputs (the cached prompt row under every sample),
 * records `consumed`, runs the existing step (all-reduce included when a communicator exists).  A staged batch is taken by ONE step or forward: stepping a
 * slot twice, or before it is staged, is refused.  arp_ft_feed_collect waits for the head's stream and reads the step's aux4 (as arp_ft_train_step).
 * arp_ft_feed_forward: the same staging, then arp_ft_forward (the reference's valid_epoch).  No hipGraph anywhere: two streams ordered by events. */
int arp_ft_feed_attach(arp_ft* h, arp_clip* towers, arp_ds* ds, const int32_t* tokens);
int arp_ft_feed_detach(arp_ft* h);
int arp_ft_feed_stage_async(arp_ft* h, int slot, const int64_t* idx, int B);
int arp_ft_feed_train_step_async(arp_ft* h, int slot, float lr);
int arp_ft_feed_collect(arp_ft* h, float* aux4);
int arp_ft_feed_forward(arp_ft* h, int slot, float* metrics4, float* scores, float* logits);

/* ---- row N4: a device-resident rollout session ------------------------------------------------------
 * batch_rollout's inner loop (arp_dt/envs/rollout_procgen.py:96-166, driven by create_test_step, main_procgen.py:171-229) for n_envs independent
 * environments: per step one uint8 frame [H, W, 3] per environment goes in and one greedy action comes out, with ONE host synchronisation.  The session keeps,
 * in HBM, a ring of the last `window` encodings, actions and returns-to-go per environment, the current return-to-go and the episode length; a step encodes
 * only the NEW frames (the frozen encoder attached to `policy`, on its latency path where that applies), builds the policy's batch on the device -- the
 * L = min(steps since reset + 1, window) real steps at the FRONT in time order, zeros behind: prepare_input's short windows at the start of an episode --
 * runs the policy's own forward and takes the argmax of the logits row L - 1.  With a reward handle the CLIP reward of the same frames
 * (get_torch_clip_reward, envs/vl_reward.py:11-23, with the handle's prompt reduction) is computed beside that on the reward handle's stream and a kernel
 * applies rtg -= (r - (use_normalize ? reward_min : 0)) / scale (:152-155); without one, `rewards` (any of VL_REWARD_FNS, computed by the caller) does, and
 * with neither the return-to-go stays constant.  H and W must be the encoder's img_res.  The policy must have a frozen encoder attached (model BC, which
 * refuses one: arp_rollout_create_with_encoder).  After a step that failed behind its first launch the session refuses further steps.  The policy and reward handles stay the caller's and must outlive the session; a session call
 * must not run beside another host thread's call on either handle. */
typedef struct arp_rollout arp_rollout;
int arp_rollout_create(arp_dt* policy, arp_clip* reward_or_null, int n_envs, int H, int W, float scale, arp_rollout** out);
/* The same with the session's encoder passed in instead of read from the policy handle.  This is how model BC runs (two tokens per step, no return-to-go
 * ring): a BC handle refuses arp_dt_attach_encoder, and goes on refusing it -- the session only borrows `encoder` for its own passes, and its geometry must be
 * the policy's enc_tokens x enc_dim.  For a BC policy a reward handle, arp_rollout_set_reward_norm and `rewards` in arp_rollout_step are refused with an
 * error string (BC.encode reads no return-to-go), and "rtg_window" does not exist. */
int arp_rollout_create_with_encoder(arp_dt* policy, arp_enc* encoder, arp_clip* reward_or_null, int n_envs, int H, int W, float scale, arp_rollout** out);
/* The same with the FINE-TUNED reward (get_torch_clip_adapter_reward, envs/vl_reward.py:44-61): at the place of the plain CLIP pass the step enqueues
 * arp_ft_reward_dev_async(head, towers, ..., transform = label) on the towers' stream; events, the return-to-go kernel and use_normalize / reward_min are
 * unchanged, `rewards` is refused as for any session that owns a reward source, and model BC refuses this reward source too.  encoder_or_null as the two
 * constructors above.  The head's prompts (arp_ft_reward_set_text, arp_ft_reward_set_reduce) may be set before or after creation, and must be current at
 * every step.  Refused at creation: towers and head on different devices or of different geometry, a goal_conditioned head. */
int arp_rollout_create_ft(arp_dt* policy, arp_enc* encoder_or_null, arp_clip* towers, arp_ft* head, int n_envs, int H, int W, float scale, arp_rollout** out);
/* A session that carries ONE GOAL FRAME PER ENVIRONMENT in HBM (the reference fixes it per episode and re-attaches it to every observation,
 * envs/rollout_procgen.py:94,108,130).  The three constructors above keep refusing a GCBC policy; this one accepts
 *   - a GCBC policy (no reward handle, as for BC; the encoder attached to it or a lent one): a step encodes the E new (frame, goal) pairs, F = (2 P + 1) x width
 *     per ring entry, and is otherwise the BC step;
 *   - an ARP-DT policy with a plain labelling handle: the reward is clip_goal_conditioned (get_torch_clip_goal_conditioned_reward, envs/vl_reward.py:26-41),
 *     reward[e] = -|| f(frame_e) - f(goal_e) ||_2 on un-normalised image features through the label transform, computed on the reward handle's stream; the
 *     goals' features are computed once, at arp_rollout_reset_goal.  No prompt set is needed; use_crop = 1 in arp_rollout_step is refused.
 * Refused: model BC, an ARP-DT policy without a reward handle, a fine-tuned head (there is no argument for one).
 * arp_rollout_reset_goal is arp_rollout_reset (rtg0_or_null: NULL for a GCBC policy, required otherwise) plus the goal frames of the listed environments, uint8
 * [n, H, W, 3] in host memory; a plain arp_rollout_reset keeps an environment's goal.  arp_rollout_step is refused until every environment has a goal.
 * arp_rollout_read gains "goal" uint8 [E, H, W, 3] and, with the goal reward, "goal_feat" f32 [E, embed]. */
int arp_rollout_create_gc(arp_dt* policy, arp_enc* encoder_or_null, arp_clip* reward_or_null, int n_envs, int H, int W, float scale, arp_rollout** out);
/* A session for model BC (InstructRL) WITH the game's instruction: tokens int32 [L], mask f32 [L] (> 0 = padded).  A step encodes the E new frames with the
 * encoder's image + text pass (arp_enc_forward_text's) under that instruction; the per-position encoding ring stays valid because the instruction is constant
 * over the episode.  encoder_or_null: the encoder to use, or NULL for the one the policy carries from arp_dt_attach_text_encoder; it must hold the text
 * weights, and the policy's enc_tokens must be 1 + P + L.  Refused for ARP-DT and GCBC policies.  No reward handle, no return-to-go (BC reads none).  The
 * existing constructors are unchanged, the image-only BC session (arp_rollout_create_with_encoder) included. */
int arp_rollout_create_text(arp_dt* policy, arp_enc* encoder_or_null, int n_envs, int H, int W, const int32_t* tokens, const float* mask, int L, arp_rollout** out);
int arp_rollout_reset_goal(arp_rollout* h, const int32_t* env_ids, int n, const float* rtg0_or_null, const uint8_t* goals_u8 /* [n, H, W, 3] */);
int arp_rollout_destroy(arp_rollout* h);
/* start an episode in the n listed environments: return-to-go rtg0[i] (already divided by scale, as :90), episode length 0 */
int arp_rollout_reset(arp_rollout* h, const int32_t* env_ids, int n, const float* rtg0);
int arp_rollout_set_lut(arp_rollout* h, const float* lut768); /* lut[c * 256 + u]: the f32 value of byte u in channel c (as arp_ds_set_lut); required */
int arp_rollout_set_reward_norm(arp_rollout* h, int use_normalize, float reward_min);
int arp_rollout_step(arp_rollout* h, const uint8_t* frames_host /* [E, H, W, 3] */, const float* rewards_or_null /* [E] */, int use_crop,
                     int32_t* actions_out /* [E] */);
/* test / logging accessor; synchronises.  what: "enc_window" f32 [E, T, tokens, dim], "action_window" int32 [E, T], "rtg_window" f32 [E, T] (the policy batch of
 * the last step), "len" int32 [E] (steps since reset), "rtg" f32 [E], "reward" f32 [E] (last step), "logits" f32 [E, T, n_actions], "enc_ring" f32
 * [T, E, tokens, dim] (slot-major), "head" int32 (the slot the next step writes).  bytes must be the item's size. */
int arp_rollout_read(arp_rollout* h, const char* what, void* out, int64_t bytes);
/* test hook: the value the window kernel writes into the padded tail (time steps L .. T - 1: encodings and return-to-go) and its action id; default 0, 0 */
int arp_rollout_debug_set_tail(arp_rollout* h, float value, int action);

/* ---- host I/O of path (1) (no GPU involved) -------------------------------
 * Reads n stored chunks of a gzip-chunked dataset (`ob` of data/PPG/trajectory_recorder.py:148-176: one chunk = one row =
 * num_frames frames) from file descriptor fd at addr[i] (size[i] bytes as stored; 0 = never written), inflates them on
 * `threads` native threads (<= 0: one per hardware thread) and copies the LAST cnt[i] frames of chunk i to out + dst_off[i].
 * stored_raw[i] != 0 (may be NULL): the deflate filter was skipped for that chunk.  Replaces the inflate half of
 * g[img_key][traj, -1] (arp_dt/label_reward.py:268); chunk addresses come from libhdf5 (arp_amd/h5store.py). */
int arp_h5_inflate_last_frames(int fd, int n, const uint64_t* addr, const uint64_t* size, const uint8_t* stored_raw,
                               uint64_t chunk_bytes, uint64_t frame_bytes, const uint64_t* dst_off, const uint32_t* cnt,
                               uint8_t* out, int threads);
/* Reward datasets of label_reward.py:273-289 (gzip chunks of ONE row): rows [first_row, first_row + n_rows) of a dataset whose chunk
   is (1, row...) are deflated here with one reused zlib stream and placed with H5Dwrite_chunk -- `write_chunk_fn` is that function's
   address inside the libhdf5 the caller has loaded (hid_t = int64, HDF5 >= 1.10.3).  `level` = the dataset's deflate level. */
int arp_h5_write_rows_deflated(void* write_chunk_fn, int64_t dset, int64_t dxpl, const void* rows, uint64_t row_bytes, uint64_t n_rows,
                               uint64_t first_row, int ndim, int level);

/* ---- single-operator entry points (host buffers; used by the per-kernel parity tests) ---------- */
/* out[M,N] = act(A[M,K] . W[N,K]^T + bias) (+ resid), operands rounded to bf16 in ARP_MODE_BF16. */
/* fp8 (e4m3) instances of the 256x256 GEMM: operands rounded to e4m3 on the host; f32 output (+ residual) or e4m3 output
 * (out_scale * act(...), returned decoded); out_fp8 = 2: IEEE-half output (the in_proj of the fp8 attention projections, returned
 * decoded).  K % 128 == 0, N % 16 == 0. */
int arp_op_gemm_fp8(int act, const float* A, const float* W, const float* bias, const float* resid, float* out, int M, int N, int K, float alpha,
                    int out_fp8, float out_scale);
int arp_op_gemm_nt(int mode, int act, const float* A, const float* W, const float* bias, const float* resid,
                   float* out, int M, int N, int K);
/* The latency path's GEMM (csrc/skinny.h: W-tiled, M <= 1024 rows, N % 16, K % 32, 16-bit modes), the kernel behind the single-frame
 * reward (reference call site: arp_dt/envs/vl_reward.py:11-23).  ksplit = 0: one launch, out = act(A.W^T + bias) + resid;
 * ksplit >= 1 (K % (32 ksplit) == 0): split-K slabs + row kernel, out = resid + bias + A.W^T, and h_out = LayerNorm(out; ln_w, ln_b, eps)
 * rounded to the operand type when ln_w != NULL. */
int arp_op_skinny_gemm(int mode, int act, const float* A, const float* W, const float* bias, const float* resid, float* out, int M, int N, int K,
                       int ksplit, const float* ln_w, const float* ln_b, float eps, float* h_out);
/* Kernels of the policy train step (16-bit modes; reference math: arp_dt/ARPDT.py:462-484 and its autodiff).
 * arp_op_gemm_tn: C[M,N] = alpha * sum_k A[k,m] B[k,n], A [K,M] and B [K,N] row-major (weight gradients dW = dY^T X);
 *   tile256 = 0: 128x128 tiles (M, N % 128), 1: 256x256 tiles (M, N % 256); K % 64; ksplit >= 1 K-slices.
 * arp_op_gemm_relu_bwd: out = (A . W^T) * (mask > 0) rounded to the operand type, colsum[N] = column sums of out (N % 8, K % 64).
 * arp_op_adapter_dy: dApre[R, tokens*D] = sigmoid(rw) * (dz[R,E] . Wi[E, tokens*D]) * (A > 0), colsum[D] = sums of dApre over rows
 *   and tokens, dres[0] = sum (dz . Wi) * (A - x); E in {32, 64, 128}, D % 128 == 0. */
int arp_op_gemm_tn(int mode, int tile256, int ksplit, const float* A, const float* B, float* out, int M, int N, int K, float alpha);
int arp_op_gemm_relu_bwd(int mode, const float* A, const float* W, const float* mask, float* out, float* colsum, int M, int N, int K);
/* The backward products of the two trainers and the reduce that finishes them (tests/test_backward_gemms_gpu.py).
 * arp_op_splitk_reduce: out[m,n] = act(alpha * sum_s part[s,m,n] + bias[n]) (+ resid[m,n]) through the product's own launcher (which picks the
 *   narrow or the 4-wide kernel), stored as out_type (ARP_MODE_F32 / BF16 / F16).  part [S][M][N]; bias, resid optional; act = 0 none, 2 ReLU,
 *   3 tanh; out and resid are [M, ldo ? ldo : N] (ldo = 0: dense).  out is uploaded before the launch and returned whole, widened to f32.
 * arp_op_gemm_bwd: kind 0 / 1 = the TN product C = alpha * A^T B (A [K, lda], B [K, ldb]) on the 128- / 256-tile kernel, written directly
 *   (ksplit == 1) or as K-slice slabs + reduce, f32 out, no resid; kind 2 = the NN product C = alpha * A B (+ resid) (A [M, lda], B [K, ldb]:
 *   dX = dY . W on a weight as it lies in memory), always slabs + reduce, out_type f32 / bf16 / f16.  mode = the operand type; the shape
 *   requirements (and the 16-bit-only rule) are the launchers' own: a refused call returns non-zero with out as it went in.  slabs (optional,
 *   ksplit * M * N + 128 * N floats): prefilled by the caller, returned as it stood between the GEMM and the reduce -- the raw slabs and 128
 *   guard rows of N behind the last. */
int arp_op_splitk_reduce(int out_type, const float* part, int S, int M, int N, const float* bias, int act, const float* resid, float* out, int ldo,
                         float alpha);
int arp_op_gemm_bwd(int kind, int mode, int out_type, int ksplit, const float* A, int lda, const float* B, int ldb, const float* resid, float* out,
                    int ldo, float* slabs, int M, int N, int K, float alpha);
int arp_op_adapter_dy(int mode, const float* dz, const float* Wi, const float* A, const float* x, float rw, float* dApre, float* colsum,
                      float* dres, int R, int E, int tokens, int D);
/* Times `iters` launches of the GEMM on device-resident random operands (HIP events); kernel: 1 = 128x128,
 * 2 = 256x256 pipelined, 0 = auto.  act/resid/out_f32 select the epilogue.  Returns the average ms per launch. */
/* ARP_MODE_F16C's product alone (gemm256 MIXC): A [M,K], W [N,K] f32 -> operand rows [rn16 | e2m1 segments] built on the host exactly as the encoder's
   kernels build them, out = A.W^T + bias (f32) with the weight rounding (plan 1) or both operand roundings (plan 2) corrected on the scaled fp4 MFMA;
   plan 0 = the plain binary16 product.  sd_sw[2] (optional): the power-of-two exponents of the e2m1 weight segments.  K % 256, N % 8. */
int arp_op_gemm_f16c(int plan, const float* A, const float* W, const float* bias, float* out, int M, int N, int K, int* sd_sw);
/* One launch of a GEMM instance the product itself launches, selected by name, on DEVICE buffers (arp_dev_malloc), through the tower's own routing
 * (tower.h::tower_gemm, or arp_enc.hip::gemm_c for the f16c names).  Synchronises before it returns.  Names and instances (T = the mode's 16-bit type):
 *   "vit.qkv" <T,T,none>  "vit.c_fc" <T,T,QuickGELU>  "vit.out_proj" / "vit.c_proj" <T,f32,none,+resid>            (the CLIP towers)
 *   "m3ae.qkv" <T,T,none>  "m3ae.c_fc" <T,T,tanh-GELU>  "m3ae.out_proj" / "m3ae.c_proj" <T,f32,none,+resid>        (the M3AE encoder)
 *   "m3ae.x3.c_fc" <f16,f32,tanh-GELU> (split3 producer of ARP_MODE_F16X3)
 *   "m3ae.f16c.c_fc" <f16,f16,tanh-GELU,MIXC>  "m3ae.f16c.c_proj" <f16,f32,none,+resid,MIXC>                       (ARP_MODE_F16C; A / W are operand rows)
 * Strides are in elements of the buffer's own type (0 = dense); ldxb as GemmArgs::ldxb.  force = TowerCtx::gemm_force (0 auto, 1 / 2 / 3). */
typedef struct arp_gemm_site {
    const char* name;
    int mode, force;
    int M, N, K, lda, ldr, ldo;
    const void* A;
    const void* W;
    const float* bias;
    const float* resid;
    void* out;
    const float* ln_stats; /* folded LayerNorm, consumer: [M][ln_parts][2] partial (sum, sum of squares), c[N], eps (1 / K is the width) */
    const float* ln_c;
    int ln_parts;
    float ln_eps;
    void* xb_out;          /* producer: operand-type copy ([hi | lo | hi] with split3) and per-128-column stats of the f32 output */
    int ldxb, split3;
    float* stats_out;
    int plan, sd, sw;      /* f16c: correction plan of the weight rows and their e2m1 scales (2^sd, 2^sw) */
    void* x4_out;          /* f16c c_fc: the e2m1 segments of the next product's operand rows (ld4 bytes per row) */
    void* dx4_out;
    int ld4;
} arp_gemm_site;
int arp_op_gemm_site(const arp_gemm_site* d);
int arp_op_gemm_bench(int mode, int kernel, int act, int resid, int out_f32, int M, int N, int K, int iters, float* avg_ms);
int arp_op_layernorm(const float* x, const float* w, const float* b, float* out, int rows, int D, float eps);
/* qkv [B*N, 3*D] -> out [B*N, D]; impl 0 = MFMA (bf16 mode, head_dim 64 only), 1 = VALU. */
int arp_op_attention(int mode, int impl, const float* qkv, float* out, int B, int N, int D, int heads, int causal);
/* Everything the product's attention launcher takes (csrc/tower.h::launch_attention): nq (query rows produced per sample; 0 = N) and the output form.
 * `out` is a raw byte buffer of out_bytes >= B * N rows which the CALLER fills: it is uploaded before the launch and downloaded after it, also when the
 * launcher refuses (its error is returned unchanged), so the caller sees every byte the kernel did not write.  Rows per form:
 *   ARP_ATTN_OUT_PLAIN   D values of the mode's type (f32 / bf16 / binary16)
 *   ARP_ATTN_OUT_E4M3    D bytes, e4m3 of out_scale * value                                 (16-bit modes, the MFMA kernel)
 *   ARP_ATTN_OUT_F16C    3 D bytes [hi: binary16 x D | x4: e2m1 x D | dx4: e2m1 x D]        (ARP_MODE_F16, the MFMA kernel); outc as the encoder passes it:
 *                        1 or 2, + 4 = no dx4 segment.  With outc & 3 == 2 the entry permutes V's columns as the encoder's weight loader does, under the
 *                        loader's rule (head_dim 64 and more than 64 tokens; otherwise V stays and the launch gets outc & 3 == 1): pass V unpermuted.
 *   ARP_ATTN_OUT_SPLIT3  3 D binary16 values [hi | lo | hi]                                 (ARP_MODE_F32, the MFMA kernels: impl 0 and 3) */
#define ARP_ATTN_OUT_PLAIN 0
#define ARP_ATTN_OUT_E4M3 1
#define ARP_ATTN_OUT_F16C 2
#define ARP_ATTN_OUT_SPLIT3 3
int arp_op_attention_forms(int mode, int impl, const float* qkv, void* out, size_t out_bytes, int B, int N, int D, int heads, int causal, int nq, int form,
                           float out_scale, int outc);
/* The same launcher with a KEY MASK (csrc/tower.h::launch_attention_masked -> csrc/attention_long.h: attn_long_masked_kernel in the 16-bit modes,
 * attn_long_f32_kernel's masked instance in ARP_MODE_F32; head_dim 64, 1 <= N <= 1024).  mask: n_words 32-bit words on the host, one bit per key, 1 = visible,
 * key k in bit k & 31 of word k >> 5, (N + 31) / 32 words per sample, sample b's words at mask + b * stride (stride 0: one mask shared by the call).  A hidden
 * key is out of every softmax of its sample.  Key 0 must be visible.  `out` as above (plain rows of the mode's type).  causal and form are passed on to the
 * launcher, which refuses a masked call that is causal, asks for another output form, has another head_dim or more than 1024 keys. */
int arp_op_attention_masked(int mode, const float* qkv, void* out, size_t out_bytes, int B, int N, int D, int heads, int causal, int nq, int form,
                            const uint32_t* mask, int n_words, int stride);
/* The fused QKV projection + attention kernel (csrc/qkvattn.h; 16-bit modes, head_dim 64, N <= 64, K % 64 == 0): A [B*N, K], in-proj weight W [3 D, K] and
 * bias [3 D] in the reference's order (q | k | v, D = heads * 64) -- the entry builds the head-major operands with the weight loader's own function.
 * out: caller-filled byte buffer as above, rows of D values of the mode's type. */
int arp_op_qkv_attention(int mode, const float* A, const float* W, const float* bias, void* out, size_t out_bytes, int B, int N, int K, int heads, int causal,
                         int nq);
/* ---- the towers' row kernels and the operand converters, each through the launch helper the product itself calls ----
 * Every output is a raw byte buffer the CALLER fills, uploaded before the launch and downloaded after it (also when the launcher refuses: its error is
 * returned unchanged), so the caller sees every byte the kernel did not write.
 *
 * arp_op_layernorm_forms: out[r] = LayerNorm(x[r * in_stride .. + D]; w, b, eps) in one of the output forms the product instantiates.  out_stride counts
 * elements of the form's storage type (the unit the product passes):
 *   ARP_LN_OUT_F32 / BF16 / F16   D values of 4 / 2 / 2 bytes
 *   ARP_LN_OUT_E4M3               D bytes, e4m3 (round to nearest even, saturating at +-448)
 *   ARP_LN_OUT_SPLIT3             3 D binary16 values [hi | lo | hi]; refused unless 3 D % 64 == 0, the K rule of the binary16 GEMM that reads the rows
 *   ARP_LN_OUT_F16C / F16C2       3 D bytes = 3 D / 2 binary16 units [hi: binary16 x D | x4: e2m1 x D | dx4: e2m1 x D]; F16C leaves the dx4 bytes alone;
 *                                 refused unless D % 256 == 0 (the rule of the f16c encoder's GEMM launcher)
 * D % 4 == 0 and D <= 2048 (the launcher's rule); strides are multiples of 4 elements.  x holds x_floats floats.  row_idx != NULL (f32, bf16, binary16
 * forms): row r reads x[row_idx[r] * in_stride ..] on the gathered kernel (the text tower's EOT rows). */
#define ARP_LN_OUT_F32 0
#define ARP_LN_OUT_BF16 1
#define ARP_LN_OUT_F16 2
#define ARP_LN_OUT_E4M3 3
#define ARP_LN_OUT_SPLIT3 4
#define ARP_LN_OUT_F16C 5
#define ARP_LN_OUT_F16C2 6
int arp_op_layernorm_forms(int form, const float* x, size_t x_floats, size_t in_stride, const int32_t* row_idx, const float* w, const float* b, void* out,
                           size_t out_bytes, int out_stride, int rows, int D, float eps);
/* row_stats_kernel (csrc/tower.h; 16-bit modes, D % 128 == 0): xb [rows, D] = x in the mode's type, stats [rows][D / 128][2] f32 = per-128-column
 * (sum, sum of squares). */
int arp_op_row_stats(int mode, const float* x, void* xb, size_t xb_bytes, void* stats, size_t stats_bytes, int rows, int D);
/* ViT token assembly (csrc/rowops.h): x [B * ntok, D] f32 = ln_pre(class / patch embedding + position; w, b).
 *   ARP_ASM_LNPRE      vit_assemble_lnpre_kernel: patch [B * (ntok - 1), D]; mode, S, slice_stride, h, stats unused
 *   ARP_ASM_LAT_LN1    vit_assemble_lat_kernel (16-bit modes): patch = S split-K slabs slice_stride floats apart, summed in slab order; h [B * ntok, D] in
 *                      the mode's type = LayerNorm(x; w1, b1)
 *   ARP_ASM_LAT_STATS  the same kernel's folded tail: h = x in the mode's type, stats [B * ntok][D / 16][2] f32: strip 0 = the row's (sum, sum of squares),
 *                      every other strip 0
 * S outside 1 .. 4 is refused (the kernel holds three extra slabs).  cls holds cls_floats >= D floats: the class embedding first; anything behind it is what
 * a class row would read if the kernel added slabs to it. */
#define ARP_ASM_LNPRE 0
#define ARP_ASM_LAT_LN1 1
#define ARP_ASM_LAT_STATS 2
int arp_op_vit_assemble(int mode, int tail, const float* patch, size_t patch_floats, int S, size_t slice_stride, const float* cls, size_t cls_floats,
                        const float* pos, const float* w, const float* b, const float* w1, const float* b1, void* x, size_t x_bytes, void* h, size_t h_bytes,
                        void* stats, size_t stats_bytes, int B, int ntok, int D, float eps);
/* x[r] = emb[tokens[r]] + pos[r % ctx]  (f32 [rows, D], D % 4 == 0; emb [vocab, D], pos [ctx, D]) */
int arp_op_text_embed(const int32_t* tokens, const float* emb, int vocab, const float* pos, void* x, size_t x_bytes, int rows, int ctx, int D);
/* out[b * ld + col0 + d] = x[row(b) * D + d], row(b) = rows[b], or b * row_stride when rows == NULL  (f32) */
int arp_op_rows_gather(const float* x, size_t x_floats, int D, const int32_t* rows, int row_stride, void* out, size_t out_bytes, int ld, int col0, int B);
/* f [rows, E] f32, in place: f[r] /= ||f[r]|| */
int arp_op_l2_normalize(void* f, size_t f_bytes, int rows, int E);
/* reward[r] = scale * <img[r], txt_n> / ||img[r]||  (f32) */
int arp_op_reward(const float* img, const float* txt_n, float scale, void* reward, size_t reward_bytes, int rows, int E);
/* The policy step's operand builders (csrc/dtops.h) through the function that picks between the 16- and the 4-value kernel (D % 16 == 0 or not; D % 8):
 * x f32 [rows, D] -> xb [rows, D] binary16 and xc, rows of 3 D bytes [hi | x4 | dx4]; with_dx = 0 leaves the dx4 bytes alone on the 16-value kernel (the
 * 4-value kernel always writes them).  arp_op_extract_hi: in = binary16 rows of stride ld -> out [rows, D] (D, ld % 8). */
int arp_op_convert_f16c(int with_dx, const float* x, void* xb, size_t xb_bytes, void* xc, size_t xc_bytes, int rows, int D);
int arp_op_extract_hi(const void* in, size_t in_bytes, int ld, void* out, size_t out_bytes, int rows, int D);
/* The f16x3 encoder's split pass: x f32 [rows, K] -> rows of 3 K binary16 values [hi | lo | hi], hi = rn16(x), lo = rn16(x - hi)  (K % 8 == 0) */
int arp_op_split3(const float* x, void* out, size_t out_bytes, int rows, int K);
/* The M3AE encoder's sequence assembly: x [nb, ntok, D], row 0 = cls, rows 1 .. GG = pe[b GG + p] + pos[p]; goal = 1: the next GG rows = pe[(nb + b) GG + p] +
 * pos[p] (pe [2 nb GG, D]); L > 0: the next L rows = text_emb[tok[j]] + tpos[j], tok int32 [L] or [nb, L] (per_row).  x goes up before the launch and comes
 * back after it.  Refuses D % 4 != 0, goal together with L > 0, and an id outside [0, vocab). */
int arp_op_m3ae_assemble(const float* pe, const float* cls, const float* pos, const float* text_emb, const float* tpos, const int32_t* tok, int nb, int GG, int goal,
                         int L, int per_row, int D, int vocab, float* x);
/* ---- the frame front ends, one kernel at a time, in the forms the passes launch ----
 * Every `out` is a byte buffer the caller fills; it goes up before the launch and comes back after it.  patch % 4 == 0 and res % patch == 0 throughout.
 *
 * arp_op_preprocess_forms: the Pillow-exact bicubic transform of arp_preprocess (uint8 NHWC frames [n, H, W, 3]) through build_plan(tr_start) and
 * launch_preprocess as a pass calls them.  mode 0 / 1 / 2 = f32 / bf16 / binary16; layout 0 = patch-major [n (res / patch)^2, 3 patch^2] (all modes),
 * 1 = NCHW [n, 3, res, res] (f32 only; anything else is refused).  tr_start: the largest tile tried, 1 .. 32 (the passes ask for 32 or 8).
 * info[8] receives what was chosen: [0] kernel instance (0 = the generic preprocess_kernel, 5 / 6 / 8 = preprocess_fast_kernel's KT), [1] TR, output rows
 * per workgroup, [2] kmax_h, [3] kmax_v, [4] max_rows, [5] lds_bytes, [6] 1 when the kernel stages input rows with 16-byte loads (no horizontal crop, rows
 * and frames multiples of 16 bytes), 0 when byte by byte, [7] tiles (workgroups) per frame.  ARP_PREPROCESS_GENERIC and ARP_PRE_LDS_KB apply. */
int arp_op_preprocess_forms(const uint8_t* frames, int n, int H, int W, int use_crop, int res, int patch, int mode, int layout, int tr_start, void* out,
                            int32_t* info);
/* The fine-tune transform (preprocess_bilinear_kernel) with the grid and the resize rule of a pass: patch-major output in the mode's type; a frame with
 * exactly one side at res is refused as a pass refuses it. */
int arp_op_preprocess_bilinear(const uint8_t* frames, int n, int H, int W, int res, int patch, int mode, void* out);
/* The same transform reading its frames through a row table (preprocess_bilinear_rows_kernel, the feed's): frame f of the output is row rows[f] of the
 * n_set frames [n_set, H, W, 3]; use_crop: the centre crop of side W / 2 as the kernel's source window.  A row outside the set is refused on the host. */
int arp_op_preprocess_bilinear_rows(const uint8_t* set_frames, int n_set, const int32_t* rows, int n, int H, int W, int use_crop, int res, int patch, int mode,
                                    void* out);
/* crop_u8_kernel: out [n, cs, cs, 3] = frames[:, y0 : y0 + cs, x0 : x0 + cs, :], the window inside the frame */
int arp_op_crop_u8(const uint8_t* frames, int n, int H, int W, int y0, int x0, int cs, uint8_t* out);
/* The M3AE encoder's patchify: images f32 NHWC [n, res, res, 3] -> rows "b (h p1) (w p2) c -> b (h w) (p1 p2 c)".  form 0 / 1 / 2: f32 / bf16 / binary16
 * rows of 3 patch^2 values; form 3: rows of 9 patch^2 binary16 values [hi | lo | hi], hi = rn16(x), lo = rn16(x - hi). */
int arp_op_patchify(const float* images, int n, int res, int patch, int form, void* out);
/* The rollout session's decide kernel: logits [E, T, n_actions], lens[e] = window length L in [1, T] -> actions_out[e] = argmax of row L - 1 (the lowest
 * index wins a tie, the first NaN wins: numpy.argmax). */
int arp_op_rollout_decide(const float* logits, const int32_t* lens, int E, int T, int n_actions, int32_t* actions_out);

#ifdef __cplusplus
}
#endif
#endif /* ARP_HIP_H */
