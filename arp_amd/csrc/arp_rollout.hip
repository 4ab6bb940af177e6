// the rollout loop (arp_dt/envs/rollout_procgen.py:96-166, driven by create_test_step, main_procgen.py:171-229) as a session whose
// state lives in HBM: one uint8 frame per environment in, one greedy action out, one host synchronisation per step.
//
// Per step, on the policy handle's stream S (E = environments, T = the policy's window):
//   upload (pinned staging) -> ingest (uint8 -> lut[c][u] f32 NHWC) -> frozen encoder on the E NEW frames only, straight into ring slot `head`
//   -> window kernel (fills the policy's synchronous batch slot: the L = min(steps since reset + 1, T) real steps at the FRONT in time order, zeros
//   behind) -> the policy's own forward (dt_internal.h) -> decide kernel (argmax of the logits row L - 1, into the action ring and the result).
// The reward pass (arp_clip_label_dev_async on the device copy of the same uint8 frames) runs on the CLIP handle's stream beside all that; a kernel
// behind it takes the reward off the return-to-go.  The two streams are ordered by events only (ev_up: frames landed; ev_win: this step's window
// kernel has read the return-to-go; ev_rtg: the return-to-go is updated and the frames are free): the host waits once, for the actions.
//
// A session made by arp_rollout_create_gc also holds one GOAL frame per environment (the reference fixes it per episode, :94, and re-attaches it to every
// observation, :108,130).  Model GCBC: the encoder pass above becomes the goal-conditioned one on the E new (frame, goal) pairs, everything else is the BC step.
// A session made by arp_rollout_create_text (model BC, InstructRL) holds the game's instruction: the encoder pass is the image + text one on the E new frames.
// An ARP-DT policy with a plain labelling handle: the reward pass becomes the features of the E new frames and a kernel that writes -||f - g||_2 against the
// goals' features, which were computed at arp_rollout_reset_goal (clip_goal_conditioned, envs/vl_reward.py:26-41).
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/arp_hip.h"
#include "clip_internal.h"
#include "common.h"
#include "dt_internal.h"
#include "enc_internal.h"
#include "ft_internal.h"
#include "runtime.h"

using namespace arp;

namespace {

// out[p] = lut[c][frames[p]]: four pixels (12 bytes in, three 16-byte stores out) per thread; n4 = pixels / 4
__global__ __launch_bounds__(256) void rollout_ingest_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ lut, float* __restrict__ out,
                                                             size_t n4) {
    __shared__ float s_lut[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += 256) s_lut[i] = lut[i];
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(frames) + i * 3;
        const uint32_t w0 = src[0], w1 = src[1], w2 = src[2];
        const uint8_t b[12] = {(uint8_t)w0, (uint8_t)(w0 >> 8), (uint8_t)(w0 >> 16), (uint8_t)(w0 >> 24), (uint8_t)w1, (uint8_t)(w1 >> 8),
                               (uint8_t)(w1 >> 16), (uint8_t)(w1 >> 24), (uint8_t)w2, (uint8_t)(w2 >> 8), (uint8_t)(w2 >> 16), (uint8_t)(w2 >> 24)};
        float4* dst = reinterpret_cast<float4*>(out) + i * 3;
#pragma unroll
        for (int q = 0; q < 3; ++q)  // byte j of the twelve belongs to channel j % 3
            dst[q] = make_float4(s_lut[((4 * q) % 3) * 256 + b[4 * q]], s_lut[((4 * q + 1) % 3) * 256 + b[4 * q + 1]],
                                 s_lut[((4 * q + 2) % 3) * 256 + b[4 * q + 2]], s_lut[((4 * q + 3) % 3) * 256 + b[4 * q + 3]]);
    }
}

struct WindowArgs {
    const float* ring;        // [T][E][F] encodings, F = tokens * dim
    const int32_t* act_ring;  // [T][E]
    float* rtg_ring;          // [T][E] (null: model without a return-to-go)
    const float* rtg_cur;     // [E]
    const int32_t* len;       // [E] steps since reset, this one not counted
    float* enc32;             // the policy's batch slot: [E][T][F], [E][T], [E][T]
    int32_t* action;
    float* rtg;
    int E, T, head;
    size_t F4;                // F / 4
    float tail;               // value of the padded tail (0; the test hook sets junk)
    int32_t tail_action;
};
// blockIdx.y = e * T + j: time position j of environment e.  j < L: ring slot (head - (L - 1 - j)) mod T; j >= L: the padded tail.
__global__ __launch_bounds__(256) void rollout_window_kernel(WindowArgs a) {
    const int e = blockIdx.y / a.T, j = blockIdx.y - e * a.T;
    const int L = min(a.len[e] + 1, a.T);
    const bool real = j < L;
    const int slot = real ? (a.head - (L - 1 - j) + a.T) % a.T : 0;
    float4* dst = reinterpret_cast<float4*>(a.enc32) + ((size_t)e * a.T + j) * a.F4;
    const float4* src = reinterpret_cast<const float4*>(a.ring) + ((size_t)slot * a.E + e) * a.F4;
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, di = (size_t)gridDim.x * 256;
    if (real) {
        for (size_t i = i0; i < a.F4; i += di) dst[i] = src[i];
    } else {
        for (size_t i = i0; i < a.F4; i += di) dst[i] = make_float4(a.tail, a.tail, a.tail, a.tail);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const bool cur = j == L - 1;  // the current step: action 0 (prepare_input's np.zeros(1)) and the return-to-go held now
        a.action[e * a.T + j] = real ? (cur ? 0 : a.act_ring[slot * a.E + e]) : a.tail_action;
        if (a.rtg) {
            const float r = real ? (cur ? a.rtg_cur[e] : a.rtg_ring[slot * a.E + e]) : a.tail;
            a.rtg[e * a.T + j] = r;
            if (cur) a.rtg_ring[a.head * a.E + e] = r;  // update_input: the step keeps the return-to-go it was decided under
        }
    }
}

// Greedy action per environment: argmax over n_actions of the logits row at time index L - 1 (lowest index on a tie, the first NaN wins: numpy.argmax).
// len_is_L: `len` holds L itself (the op entry); otherwise steps since reset, and the kernel advances it.  act_slot: the action ring's current slot or null.
__global__ __launch_bounds__(64) void rollout_decide_kernel(const float* __restrict__ logits, int32_t* len, int len_is_L, int E, int T, int NA,
                                                            int32_t* act_slot, int32_t* actions_out) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    const int L = len_is_L ? len[e] : min(len[e] + 1, T);
    const float* row = logits + ((size_t)e * T + (L - 1)) * NA;
    int best = 0;
    float bv = row[0];
    if (!(bv != bv)) {
        for (int i = 1; i < NA; ++i) {
            const float v = row[i];
            if (v != v) { best = i; break; }
            if (v > bv) { bv = v; best = i; }
        }
    }
    actions_out[e] = best;
    if (act_slot) act_slot[e] = best;
    if (!len_is_L) len[e] = len[e] + 1;
}

// rtg[e] -= (reward[e] - sub) / scale   (rollout_procgen.py:152-155; sub = use_normalize ? reward_min : 0)
__global__ __launch_bounds__(64) void rollout_rtg_kernel(float* __restrict__ rtg, const float* __restrict__ reward, float sub, float scale, int E) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e < E) rtg[e] -= (reward[e] - sub) / scale;
}

// The goal reward (get_torch_clip_goal_conditioned_reward, envs/vl_reward.py:26-41): reward[e] = -|| f[e] - g[e] ||_2 on un-normalised image features.  One wave
// per environment, f32; lane l sums elements l, l + 64, ... in index order and the lanes are folded by a fixed xor butterfly, so a value depends on its two rows
// and on nothing else (not on E, not on the other environments).
__global__ __launch_bounds__(64) void rollout_goal_reward_kernel(const float* __restrict__ f, const float* __restrict__ g, int D, float* __restrict__ reward) {
    const int e = blockIdx.x, lane = threadIdx.x;
    const float* fr = f + (size_t)e * D;
    const float* gr = g + (size_t)e * D;
    float acc = 0.f;
    for (int i = lane; i < D; i += 64) {
        const float d = fr[i] - gr[i];
        acc += d * d;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) reward[e] = -sqrtf(acc);
}

// reset of the listed environments: return-to-go, episode length
__global__ __launch_bounds__(64) void rollout_reset_kernel(const int32_t* __restrict__ ids, const float* __restrict__ rtg0, int n, float* rtg, int32_t* len) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    rtg[ids[i]] = rtg0[i];
    len[ids[i]] = 0;
}

}  // namespace

struct arp_rollout {
    arp_dt* dt = nullptr;
    arp_clip* clip = nullptr;
    arp_ft* ft = nullptr;  // the fine-tuned reward: `clip` is then its towers (arp_rollout_create_ft)
    arp_enc* enc = nullptr;
    DtRolloutInfo pi{};
    hipStream_t clip_stream = nullptr;
    int E = 0, H = 0, W = 0;
    float scale = 1.f;
    int use_normalize = 0;
    float reward_min = 0.f;
    size_t F = 0;  // floats per encoding
    DevBuf frames_u8, enc_in, ring, act_ring, rtg_ring, rtg_cur, len, reward, actions, lut, reset_ids, reset_rtg;
    PinBuf pin_frames, pin_small;  // pin_small: [E] rewards in, [E] actions out
    bool enqueued = false;  // the running step has launched something
    bool broken = false;    // a step failed behind its first launch
    Event ev_up, ev_win, ev_rtg;
    bool rtg_pending = false;  // ev_rtg has been recorded behind work the compute stream has not waited for yet
    bool has_lut = false, any_reset = false;
    int head = 0;  // the ring slot the NEXT step writes
    float tail = 0.f;
    int32_t tail_action = 0;
    // A session made by arp_rollout_create_gc carries one goal frame per environment: uint8 as it came; for a GCBC policy also f32 through the byte -> float table
    // (the encoder's second input); for an ARP-DT policy with a labelling handle the goals' un-normalised CLIP image features (the goal reward).
    bool gc = false;
    int embed = 0;                  // the reward handle's feature width (goal reward)
    DevBuf goals_u8, goal32, goal_feat, frame_feat;
    std::vector<char> has_goal;     // [E]
    bool goal_reward() const { return gc && clip; }
    // A session made by arp_rollout_create_text (model BC, InstructRL): the instruction its steps encode the E new frames with.  Constant over the episode, so a
    // ring entry stays valid for as long as its frame is in the window.
    EncText text;
    const float* logits = nullptr;  // the policy's logits buffer as of the last step
    float* slot_enc = nullptr;
    int32_t* slot_action = nullptr;
    float* slot_rtg = nullptr;
};
static_assert(!std::is_copy_constructible_v<arp_rollout>);

namespace {

int quiesce(arp_rollout* s) {
    ARP_HIP_OK(hipSetDevice(s->pi.device));
    ARP_HIP_OK(hipStreamSynchronize(s->pi.stream));
    if (s->clip_stream) ARP_HIP_OK(hipStreamSynchronize(s->clip_stream));
    s->rtg_pending = false;
    return 0;
}

}  // namespace

extern "C" {

static int rollout_create(arp_dt* policy, arp_enc* encoder, arp_clip* reward, arp_ft* head, int n_envs, int H, int W, float scale, arp_rollout** out,
                          bool gc = false, int text_L = 0) {
    if (!policy || !out) return fail("null argument");
    if (n_envs <= 0) return fail("rollout: n_envs must be positive");
    if (!(scale != 0.f)) return fail("rollout: scale must not be zero");
    auto s = std::make_unique<arp_rollout>();
    ARP_TRY(dt_rollout_info(policy, &s->pi));
    if (s->pi.gcbc && !gc) return fail("rollout: model GCBC needs a goal frame per episode, which a session does not carry");
    if (gc && head) return fail("rollout: create_gc takes a plain labelling handle: the fine-tuned goal reward stays with the host function");
    if (gc && s->pi.bc && !s->pi.gcbc) return fail("rollout: create_gc: model BC reads no goal frame (model GCBC does)");
    if (gc && !s->pi.bc && !reward) return fail("rollout: create_gc: an ARP-DT policy carries goal frames for the goal reward only: pass a labelling handle");
    // Model BC refuses arp_dt_attach_encoder (its reference encoder reads the instruction's text tokens too; arp_rollout_create_text is the session that
    // carries them): a session without an instruction is LENT an encoder for its own
    // passes (arp_rollout_create_with_encoder); the handle's refusal stands.  BC.encode reads no return-to-go: no ring, no reward source.
    if (encoder) s->pi.enc = encoder;
    if (!s->pi.enc)
        return fail(s->pi.bc ? "rollout: model BC cannot have an encoder attached: pass one to arp_rollout_create_with_encoder"
                             : "rollout: the policy handle has no frozen encoder attached (arp_dt_attach_encoder)");
    if (s->pi.bc && reward) return fail("rollout: model BC reads no return-to-go: a reward handle is refused");
    int tokens = 0, width = 0, res = 0, dev = 0;
    ARP_TRY(enc_geometry(s->pi.enc, &tokens, &width, &res, &dev));
    if (s->pi.gcbc) ARP_TRY(enc_seq_tokens(s->pi.enc, EncSeq::goal(), &tokens));  // a (frame, goal) pair per ring entry
    if (text_L > 0) ARP_TRY(enc_seq_tokens(s->pi.enc, EncSeq::text(text_L), &tokens));  // a frame and the instruction per ring entry
    if (H != res || W != res) return fail("rollout: frames are " + std::to_string(H) + " x " + std::to_string(W) + ", the attached encoder reads " + std::to_string(res) + " x " + std::to_string(res));
    if (tokens != s->pi.enc_tokens || width != s->pi.enc_dim) return fail("rollout: encoder geometry does not match the policy's enc_tokens / enc_dim");
    if (dev != s->pi.device) return fail("rollout: the encoder lives on another device");
    if (((size_t)H * W) % 4 || ((size_t)tokens * width) % 4) return fail("rollout: H * W and tokens * width must be multiples of 4");
    if (reward && head) {  // the fine-tuned reward: the towers need no prompt set of their own, the head caches its prompts
        ARP_TRY(ft_reward_check(head, reward));
        ClipMsInfo ci;
        ARP_TRY(clip_ms_info(reward, &ci));
        if (ci.device != s->pi.device) return fail("rollout: the reward handles live on another device");
        s->clip_stream = ci.stream;
    } else if (reward && gc) {  // the goal reward reads image features only: no prompt set is asked for
        ClipMsInfo ci;
        ARP_TRY(clip_ms_info(reward, &ci));
        if (ci.device != s->pi.device) return fail("rollout: the reward handle lives on another device");
        if (n_envs > ci.max_batch) return fail("rollout: the goal reward encodes n_envs frames per call: n_envs exceeds the reward handle's max_batch");
        s->clip_stream = ci.stream;
        s->embed = ci.embed;
    } else if (reward) {
        int cdev = 0;
        ARP_TRY(clip_stream_of(reward, &s->clip_stream, &cdev));
        if (cdev != s->pi.device) return fail("rollout: the reward handle lives on another device");
    }
    ARP_HIP_OK(hipSetDevice(s->pi.device));
    s->dt = policy; s->clip = reward; s->ft = head; s->enc = s->pi.enc;
    s->E = n_envs; s->H = H; s->W = W; s->scale = scale; s->gc = gc;
    s->F = (size_t)tokens * width;
    const size_t E = n_envs, T = s->pi.window, fb = (size_t)H * W * 3;
    ARP_TRY(s->frames_u8.ensure(E * fb)); ARP_TRY(s->enc_in.ensure(E * fb * 4));
    ARP_TRY(s->ring.ensure(T * E * s->F * 4)); ARP_TRY(s->act_ring.ensure(T * E * 4));
    if (!s->pi.bc) ARP_TRY(s->rtg_ring.ensure(T * E * 4));
    ARP_TRY(s->rtg_cur.ensure(E * 4)); ARP_TRY(s->len.ensure(E * 4)); ARP_TRY(s->reward.ensure(E * 4)); ARP_TRY(s->actions.ensure(E * 4));
    ARP_TRY(s->lut.ensure(3 * 256 * 4)); ARP_TRY(s->reset_ids.ensure(E * 4)); ARP_TRY(s->reset_rtg.ensure(E * 4));
    ARP_TRY(s->pin_frames.ensure(E * fb)); ARP_TRY(s->pin_small.ensure(4 * E * 4));
    if (gc) {
        s->has_goal.assign(E, 0);
        ARP_TRY(s->goals_u8.ensure(E * fb));
        if (s->pi.gcbc) ARP_TRY(s->goal32.ensure(E * fb * 4));
        if (reward) { ARP_TRY(s->goal_feat.ensure(E * s->embed * 4)); ARP_TRY(s->frame_feat.ensure(E * s->embed * 4)); }
    }
    ARP_TRY(s->ev_up.create()); ARP_TRY(s->ev_win.create()); ARP_TRY(s->ev_rtg.create());
    for (DevBuf* b : {&s->ring, &s->act_ring, &s->rtg_ring, &s->rtg_cur, &s->len, &s->reward, &s->actions, &s->goals_u8, &s->goal32, &s->goal_feat, &s->frame_feat})
        if (b->p) ARP_HIP_OK(hipMemset(b->p, 0, b->bytes));
    *out = s.release();
    return 0;
}

int arp_rollout_create(arp_dt* policy, arp_clip* reward, int n_envs, int H, int W, float scale, arp_rollout** out) {
    return rollout_create(policy, nullptr, reward, nullptr, n_envs, H, W, scale, out);
}
int arp_rollout_create_with_encoder(arp_dt* policy, arp_enc* encoder, arp_clip* reward, int n_envs, int H, int W, float scale, arp_rollout** out) {
    if (!encoder) return fail("null encoder");
    return rollout_create(policy, encoder, reward, nullptr, n_envs, H, W, scale, out);
}
int arp_rollout_create_ft(arp_dt* policy, arp_enc* encoder_or_null, arp_clip* towers, arp_ft* head, int n_envs, int H, int W, float scale, arp_rollout** out) {
    if (!towers || !head) return fail("null reward handle");
    return rollout_create(policy, encoder_or_null, towers, head, n_envs, H, W, scale, out);
}

int arp_rollout_create_gc(arp_dt* policy, arp_enc* encoder_or_null, arp_clip* reward_or_null, int n_envs, int H, int W, float scale, arp_rollout** out) {
    return rollout_create(policy, encoder_or_null, reward_or_null, nullptr, n_envs, H, W, scale, out, true);
}

// Model BC (InstructRL) with the instruction of the game: tokens int32 [L], mask f32 [L] (> 0 = padded).  The encoder is the one given, or the one the policy
// carries from arp_dt_attach_text_encoder; either way it must hold the text weights, and enc_tokens == 1 + P + L.
int arp_rollout_create_text(arp_dt* policy, arp_enc* encoder_or_null, int n_envs, int H, int W, const int32_t* tokens, const float* mask, int L, arp_rollout** out) {
    if (!policy || !tokens || !mask || !out) return fail("null argument");
    if (L <= 0) return fail("rollout: create_text: the instruction has no tokens");
    DtRolloutInfo pi{};
    ARP_TRY(dt_rollout_info(policy, &pi));
    if (!pi.bc || pi.gcbc) return fail("rollout: create_text: an instruction belongs to model BC (ARP-DT's and GCBC's encoder calls read no text)");
    arp_enc* enc = encoder_or_null ? encoder_or_null : pi.enc;
    if (!enc) return fail("rollout: create_text: no encoder (pass one, or attach one with arp_dt_attach_text_encoder)");
    ARP_HIP_OK(hipSetDevice(pi.device));
    EncText text;
    ARP_TRY(text.set(enc, tokens, mask, L));  // the text weights, the mode, the ids, the position rows: before the session exists
    arp_rollout* s = nullptr;
    ARP_TRY(rollout_create(policy, enc, nullptr, nullptr, n_envs, H, W, 1.f, &s, false, L));
    s->text = std::move(text);
    *out = s;
    return 0;
}

int arp_rollout_destroy(arp_rollout* s) {
    if (!s) return 0;
    (void)quiesce(s);
    delete s;
    return 0;
}

// uint8 -> f32 through the session's table, `frames` frames on the policy's stream
static int launch_ingest(arp_rollout* s, const uint8_t* src, float* dst, size_t frames) {
    const size_t n4 = frames * s->H * s->W / 4;
    hipLaunchKernelGGL(rollout_ingest_kernel, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 2048)), dim3(256), 0, s->pi.stream, src, s->lut.as<float>(), dst, n4);
    ARP_HIP_OK(hipGetLastError());
    return 0;
}
// a GCBC session's goals as the encoder reads them: all E at once (an environment without a goal yet holds zeros, and no step runs before it has one)
static int ingest_goals(arp_rollout* s) {
    if (!s->gc || !s->pi.gcbc || !s->has_lut) return 0;
    ARP_TRY(launch_ingest(s, s->goals_u8.as<uint8_t>(), s->goal32.as<float>(), (size_t)s->E));
    ARP_HIP_OK(hipStreamSynchronize(s->pi.stream));
    return 0;
}

int arp_rollout_set_lut(arp_rollout* s, const float* lut768) {
    if (!s || !lut768) return fail("null argument");
    ARP_TRY(quiesce(s));
    ARP_HIP_OK(hipMemcpy(s->lut.p, lut768, 3 * 256 * 4, hipMemcpyHostToDevice));
    s->has_lut = true;
    return ingest_goals(s);  // (a GCBC session's f32 goals are table values: a new table, new goals)
}

int arp_rollout_set_reward_norm(arp_rollout* s, int use_normalize, float reward_min) {
    if (!s) return fail("null handle");
    if (s->pi.bc) return fail("rollout: model BC reads no return-to-go: set_reward_norm is refused");
    s->use_normalize = use_normalize ? 1 : 0;
    s->reward_min = reward_min;
    return 0;
}

/* test hook: what the window kernel writes into the padded tail (time steps L .. T - 1) of the policy's batch -- value for encodings and return-to-go, and an
   action id.  The default, and what the reference's shorter window corresponds to, is zero. */
int arp_rollout_debug_set_tail(arp_rollout* s, float value, int action) {
    if (!s) return fail("null handle");
    if (action < 0 || action >= s->pi.n_actions) return fail("rollout: tail action out of range");
    s->tail = value;
    s->tail_action = action;
    return 0;
}

static int rollout_reset(arp_rollout* s, const int32_t* env_ids, int n, const float* rtg0, const uint8_t* goals_u8);
int arp_rollout_reset(arp_rollout* s, const int32_t* env_ids, int n, const float* rtg0) {
    if (!s || !env_ids || !rtg0) return fail("null argument");
    return rollout_reset(s, env_ids, n, rtg0, nullptr);
}
int arp_rollout_reset_goal(arp_rollout* s, const int32_t* env_ids, int n, const float* rtg0, const uint8_t* goals_u8) {
    if (!s || !env_ids || !goals_u8) return fail("null argument");
    if (!s->gc) return fail("rollout: reset_goal needs a session that carries goal frames (arp_rollout_create_gc)");
    if (!rtg0 && !s->pi.bc) return fail("rollout: reset_goal: the first return-to-go is required (only model GCBC reads none)");
    return rollout_reset(s, env_ids, n, rtg0, goals_u8);
}
static int rollout_reset(arp_rollout* s, const int32_t* env_ids, int n, const float* rtg0, const uint8_t* goals_u8) {
    if (n <= 0 || n > s->E) return fail("rollout: reset names 1 .. n_envs environments");
    for (int i = 0; i < n; ++i) {
        if (env_ids[i] < 0 || env_ids[i] >= s->E) return fail("rollout: env_id " + std::to_string(env_ids[i]) + " out of range [0, " + std::to_string(s->E) + ")");
        for (int j = 0; j < i; ++j)
            if (env_ids[j] == env_ids[i]) return fail("rollout: env_id " + std::to_string(env_ids[i]) + " listed twice");
    }
    ARP_TRY(quiesce(s));  // (a reset is rare: behind everything in flight, the return-to-go kernel of the last step included)
    ARP_HIP_OK(hipMemcpy(s->reset_ids.p, env_ids, (size_t)n * 4, hipMemcpyHostToDevice));
    if (rtg0) ARP_HIP_OK(hipMemcpy(s->reset_rtg.p, rtg0, (size_t)n * 4, hipMemcpyHostToDevice));
    else ARP_HIP_OK(hipMemset(s->reset_rtg.p, 0, (size_t)n * 4));
    hipLaunchKernelGGL(rollout_reset_kernel, dim3((n + 63) / 64), dim3(64), 0, s->pi.stream, s->reset_ids.as<int32_t>(), s->reset_rtg.as<float>(), n,
                       s->rtg_cur.as<float>(), s->len.as<int32_t>());
    ARP_HIP_OK(hipGetLastError());
    ARP_HIP_OK(hipStreamSynchronize(s->pi.stream));
    s->any_reset = true;
    if (goals_u8) {  // the listed environments' goals, then everything derived from them (both streams are idle: quiesce above)
        const size_t fb = (size_t)s->H * s->W * 3;
        for (int i = 0; i < n; ++i) {
            ARP_HIP_OK(hipMemcpy(s->goals_u8.as<uint8_t>() + (size_t)env_ids[i] * fb, goals_u8 + (size_t)i * fb, fb, hipMemcpyHostToDevice));
            s->has_goal[env_ids[i]] = 1;
        }
        ARP_TRY(ingest_goals(s));
        if (s->goal_reward()) {
            // All E goals in ONE call, as a step encodes its E frames in one call (the towers choose their kernels by the call's rows); an environment
            // whose goal did not change gets the bits it had.  Label transform, no crop, un-normalised.
            ARP_TRY(arp_clip_encode_image_dev_async(s->clip, s->goals_u8.as<uint8_t>(), s->E, s->H, s->W, 0, 0, s->goal_feat.as<float>()));
            ARP_HIP_OK(hipStreamSynchronize(s->clip_stream));
        }
    }
    return 0;
}

static int rollout_step(arp_rollout* s, const uint8_t* frames_host, const float* rewards, int use_crop, int32_t* actions_out);
int arp_rollout_step(arp_rollout* s, const uint8_t* frames_host, const float* rewards, int use_crop, int32_t* actions_out) {
    if (!s || !frames_host || !actions_out) return fail("null argument");
    if (s->broken) return fail("rollout: an earlier step failed part way: the session's state is undefined (destroy it)");
    const int rc = rollout_step(s, frames_host, rewards, use_crop, actions_out);
    if (rc != 0 && s->enqueued) {  // failed behind its first launch: drain both streams, keep the error string, refuse further steps
        const std::string msg = arp_last_error();
        (void)quiesce(s);
        s->broken = true;
        return fail(msg);
    }
    return rc;
}
static int rollout_step(arp_rollout* s, const uint8_t* frames_host, const float* rewards, int use_crop, int32_t* actions_out) {
    s->enqueued = false;
    if (!s->any_reset) return fail("rollout: step before the first reset");
    if (!s->has_lut) return fail("rollout: no byte -> float table (arp_rollout_set_lut)");
    if (rewards && s->clip) return fail("rollout: rewards were passed to a session that owns a reward handle");
    if (rewards && s->pi.bc) return fail("rollout: model BC reads no return-to-go: rewards are refused");
    if (s->gc) {
        for (int e = 0; e < s->E; ++e)
            if (!s->has_goal[e]) return fail("rollout: environment " + std::to_string(e) + " has no goal frame yet (arp_rollout_reset_goal)");
        if (s->clip && use_crop) return fail("rollout: use_crop with the device goal reward is refused (the reference crops the goal's crop again: that stays with the host function)");
    }
    ARP_HIP_OK(hipSetDevice(s->pi.device));
    const int E = s->E, T = s->pi.window, NA = s->pi.n_actions;
    const size_t fb = (size_t)s->H * s->W * 3;
    hipStream_t S = s->pi.stream;
    // the policy's batch slot (may have been re-staged by a train / validation call since the last step)
    ARP_TRY(dt_rollout_bind(s->dt, E, &s->slot_enc, &s->slot_action, &s->slot_rtg));
    // behind the last step's reward pass: it read the frame buffer and its kernel wrote the return-to-go this step's window kernel reads
    if (s->rtg_pending) {
        ARP_HIP_OK(hipStreamWaitEvent(S, s->ev_rtg, 0));
        s->rtg_pending = false;
    }
    s->enqueued = true;
    // 1. the one upload of frame data (the last step's copy out of the staging buffer finished before that step returned)
    memcpy(s->pin_frames.p, frames_host, (size_t)E * fb);
    ARP_HIP_OK(hipMemcpyAsync(s->frames_u8.p, s->pin_frames.p, (size_t)E * fb, hipMemcpyHostToDevice, S));
    float* pin_rew = s->pin_small.as<float>();
    int32_t* pin_act = s->pin_small.as<int32_t>() + E;
    if (rewards) {
        memcpy(pin_rew, rewards, (size_t)E * 4);
        ARP_HIP_OK(hipMemcpyAsync(s->reward.p, pin_rew, (size_t)E * 4, hipMemcpyHostToDevice, S));
    }
    if (s->clip) {  // 7. the reward pass, beside steps 2-6 on the labelling handle's own stream
        ARP_HIP_OK(hipEventRecord(s->ev_up, S));
        ARP_HIP_OK(hipStreamWaitEvent(s->clip_stream, s->ev_up, 0));
        if (s->gc) {
            ARP_TRY(arp_clip_encode_image_dev_async(s->clip, s->frames_u8.as<uint8_t>(), E, s->H, s->W, 0, 0, s->frame_feat.as<float>()));
            hipLaunchKernelGGL(rollout_goal_reward_kernel, dim3(E), dim3(64), 0, s->clip_stream, s->frame_feat.as<float>(), s->goal_feat.as<float>(), s->embed,
                               s->reward.as<float>());
            ARP_HIP_OK(hipGetLastError());
        } else if (s->ft) ARP_TRY(arp_ft_reward_dev_async(s->ft, s->clip, s->frames_u8.as<uint8_t>(), E, s->H, s->W, use_crop, 1 /* label transform */, s->reward.as<float>()));
        else ARP_TRY(arp_clip_label_dev_async(s->clip, s->frames_u8.as<uint8_t>(), E, s->H, s->W, use_crop, s->reward.as<float>()));
    }
    // 2. ingest
    ARP_TRY(launch_ingest(s, s->frames_u8.as<uint8_t>(), s->enc_in.as<float>(), (size_t)E));
    // 3. the encoder on the E new frames (model GCBC: on the E new (frame, goal) pairs), straight into ring slot `head`
    float* slot = s->ring.as<float>() + (size_t)s->head * E * s->F;
    const EncSeq seq = s->pi.gcbc ? EncSeq::goal(s->goal32.as<float>()) : s->text.L > 0 ? s->text.seq() : EncSeq{};  // (model BC with its instruction: the image + text pass)
    ARP_TRY(enc_forward_on(s->enc, S, s->enc_in.as<float>(), E, slot, seq, true));
    // 4. window
    {
        WindowArgs a;
        a.ring = s->ring.as<float>(); a.act_ring = s->act_ring.as<int32_t>(); a.rtg_ring = s->pi.bc ? nullptr : s->rtg_ring.as<float>(); a.rtg_cur = s->rtg_cur.as<float>();
        a.len = s->len.as<int32_t>(); a.enc32 = s->slot_enc; a.action = s->slot_action; a.rtg = s->slot_rtg;
        a.E = E; a.T = T; a.head = s->head; a.F4 = s->F / 4; a.tail = s->tail; a.tail_action = s->tail_action;
        hipLaunchKernelGGL(rollout_window_kernel, dim3((unsigned)std::min<size_t>((a.F4 + 255) / 256, 64), E * T), dim3(256), 0, S, a);
        ARP_HIP_OK(hipGetLastError());
    }
    const bool rtg_update = s->clip || rewards;
    if (s->clip) ARP_HIP_OK(hipEventRecord(s->ev_win, S));
    // 5. the policy's forward
    ARP_TRY(dt_rollout_forward(s->dt, &s->logits));
    // 6. decide
    hipLaunchKernelGGL(rollout_decide_kernel, dim3((E + 63) / 64), dim3(64), 0, S, s->logits, s->len.as<int32_t>(), 0, E, T, NA,
                       s->act_ring.as<int32_t>() + (size_t)s->head * E, s->actions.as<int32_t>());
    ARP_HIP_OK(hipGetLastError());
    ARP_HIP_OK(hipMemcpyAsync(pin_act, s->actions.p, (size_t)E * 4, hipMemcpyDeviceToHost, S));
    // 7. the return-to-go: behind the reward (its stream) and behind this step's window kernel, which read the value held so far
    if (rtg_update) {
        hipStream_t R = s->clip ? s->clip_stream : S;
        if (s->clip) ARP_HIP_OK(hipStreamWaitEvent(R, s->ev_win, 0));
        hipLaunchKernelGGL(rollout_rtg_kernel, dim3((E + 63) / 64), dim3(64), 0, R, s->rtg_cur.as<float>(), s->reward.as<float>(),
                           s->use_normalize ? s->reward_min : 0.f, s->scale, E);
        ARP_HIP_OK(hipGetLastError());
        if (s->clip) {
            ARP_HIP_OK(hipEventRecord(s->ev_rtg, R));
            s->rtg_pending = true;
        }
    }
    s->head = (s->head + 1) % T;
    ARP_HIP_OK(hipStreamSynchronize(S));  // the step's one host wait
    memcpy(actions_out, pin_act, (size_t)E * 4);
    return 0;
}

int arp_rollout_read(arp_rollout* s, const char* what, void* out, int64_t bytes) {
    if (!s || !what || !out) return fail("null argument");
    ARP_TRY(quiesce(s));
    const size_t E = s->E, T = s->pi.window;
    const std::string w(what);
    const void* src = nullptr;
    size_t n = 0;
    if (w == "enc_window") { src = s->slot_enc; n = E * T * s->F * 4; }
    else if (w == "action_window") { src = s->slot_action; n = E * T * 4; }
    else if (w == "rtg_window") {
        if (s->pi.bc) return fail("rollout read: model BC has no return-to-go");
        src = s->slot_rtg; n = E * T * 4;
    }
    else if (w == "len") { src = s->len.p; n = E * 4; }
    else if (w == "rtg") { src = s->rtg_cur.p; n = E * 4; }
    else if (w == "reward") { src = s->reward.p; n = E * 4; }
    else if (w == "logits") { src = s->logits; n = E * T * s->pi.n_actions * 4; }
    else if (w == "enc_ring") { src = s->ring.p; n = T * E * s->F * 4; }
    else if (w == "goal") {
        if (!s->gc) return fail("rollout read: goal exists on a session that carries goal frames (arp_rollout_create_gc)");
        src = s->goals_u8.p; n = E * s->H * s->W * 3;
    }
    else if (w == "goal_feat") {
        if (!s->goal_reward()) return fail("rollout read: goal_feat exists on a session with the device goal reward");
        src = s->goal_feat.p; n = E * s->embed * 4;
    }
    else if (w == "head") {
        if (bytes != 4) return fail("rollout read: head is one int32");
        *static_cast<int32_t*>(out) = s->head;
        return 0;
    } else return fail("rollout read: unknown item " + w);
    if (!src) return fail("rollout read: " + w + " exists after the first step");
    if ((size_t)bytes != n) return fail("rollout read: " + w + " is " + std::to_string(n) + " bytes");
    ARP_HIP_OK(hipMemcpy(out, src, n, hipMemcpyDeviceToHost));
    return 0;
}

int arp_op_rollout_decide(const float* logits, const int32_t* lens, int E, int T, int n_actions, int32_t* actions_out) {
    if (!logits || !lens || !actions_out || E <= 0 || T <= 0 || n_actions <= 0) return fail("bad argument");
    for (int e = 0; e < E; ++e)
        if (lens[e] < 1 || lens[e] > T) return fail("rollout_decide: lens are window lengths in [1, T]");
    DevBuf dl, dn, da;
    const size_t nl = (size_t)E * T * n_actions * 4;
    ARP_TRY(dl.ensure(nl)); ARP_TRY(dn.ensure((size_t)E * 4)); ARP_TRY(da.ensure((size_t)E * 4));
    ARP_HIP_OK(hipMemcpy(dl.p, logits, nl, hipMemcpyHostToDevice));
    ARP_HIP_OK(hipMemcpy(dn.p, lens, (size_t)E * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(rollout_decide_kernel, dim3((E + 63) / 64), dim3(64), 0, nullptr, dl.as<float>(), dn.as<int32_t>(), 1, E, T, n_actions,
                       (int32_t*)nullptr, da.as<int32_t>());
    ARP_HIP_OK(hipGetLastError());
    ARP_HIP_OK(hipDeviceSynchronize());
    ARP_HIP_OK(hipMemcpy(actions_out, da.p, (size_t)E * 4, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
