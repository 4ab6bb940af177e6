// Internal (C++) hooks that let the policy step, the dataset and the rollout session run the frozen encoder on their own streams.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "runtime.h"

struct arp_enc;
struct arp_gemm_site;
namespace arp {

// What follows the class token and the frame's P patches in a sample's sequence, P = (res / patch)^2, P1 = 1 + P.  Everything else about a pass -- chunks of
// max_frames samples, part streams, the latency rule on the call's total rows -- is the same for the three kinds and counts samples and rows of this sequence.
//   PLAIN  nothing: P1 rows (forward_representation on frames alone).
//   GOAL   the goal frame's P patches under the same position (+ type) embedding: 2 P + 1 rows per (frame, goal) pair (forward_gc_representations).  Both frame
//          sets go through patchify and ONE patch-embedding product of 2 nb P rows.  goals_dev: f32 NHWC [n, res, res, 3] in HBM.
//   TEXT   an instruction of L tokens: P1 + L rows, every attention under the instruction's key mask (tower.h: the key-blocked masked kernels at any length).
//          tok_dev: int32 ids, [L] shared by the frames or [n, L] (per_row), already checked against the vocabulary; words_dev / words_host: the
//          visible-bit words (attention_long.h's mask format) over the P1 + L keys, words(P1) per instruction, in HBM and on the host (the attention launcher
//          checks key 0 there): class and patch keys always visible, text key i visible where the caller's padding mask is <= 0.
// ARP_MODE_F16C runs PLAIN only (its [hi | x4 | dx4] attention rows exist on the LDS-resident kernel only, <= 288 tokens).
struct EncSeq {
    enum Kind { PLAIN, GOAL, TEXT } kind = PLAIN;
    const float* goals_dev = nullptr;
    const int32_t* tok_dev = nullptr;
    const uint32_t *words_dev = nullptr, *words_host = nullptr;
    int L = 0, per_row = 0;
    static EncSeq goal(const float* goals_dev = nullptr) {  // (no frames: for the row count alone, as text(L) is)
        EncSeq s;
        s.kind = GOAL; s.goals_dev = goals_dev;
        return s;
    }
    static EncSeq text(int L, int per_row = 0, const int32_t* tok_dev = nullptr, const uint32_t* words_dev = nullptr, const uint32_t* words_host = nullptr) {
        EncSeq s;
        s.kind = TEXT; s.L = L; s.per_row = per_row ? 1 : 0; s.tok_dev = tok_dev; s.words_dev = words_dev; s.words_host = words_host;
        return s;
    }
    int tokens(int P1) const { return kind == TEXT ? P1 + L : kind == GOAL ? 2 * (P1 - 1) + 1 : P1; }  // rows per sample
    int words(int P1) const { return (P1 + L + 31) / 32; }                                              // mask words per instruction
    // the workspace of this many plain frames holds nb samples: a pair is 2 P + 1 token rows and 2 P patch rows, nb instructions' frames are nb (P1 + L) token rows
    int ws_frames(int nb, int P1) const { return kind == TEXT ? (int)(((long)nb * (P1 + L) + P1 - 1) / P1) : kind == GOAL ? 2 * nb : nb; }
    // the sequence of the samples from `frame` on (frame_floats = res * res * 3)
    EncSeq at(int frame, size_t frame_floats, int P1) const {
        EncSeq s = *this;
        if (goals_dev) s.goals_dev += frame * frame_floats;
        if (per_row) { s.tok_dev += (size_t)frame * L; s.words_dev += (size_t)frame * words(P1); s.words_host += (size_t)frame * words(P1); }
        return s;
    }
};

// images_dev: f32 NHWC [n, res, res, 3] in HBM; out_dev: f32 [n * seq.tokens(P1), width].  Enqueues the pass of n samples behind everything already on `stream`;
// `stream` continues behind the last part.  Safe under a stream capture of `stream` (the part streams join the capture through the fork event and leave it
// through the join events), but every buffer must exist beforehand: the first call of a geometry (and of an instruction length, which uploads its position
// rows) allocates and must run eagerly (arp_dt.hip runs two eager steps before it captures).
// latency: the caller is a rollout step (a handful of samples, one pass per environment step): a call of at most arp_enc::lat_rows token rows IN TOTAL in the
// plain 16-bit modes then runs on tower.h's latency path.  The training paths leave it false and keep their kernels at every size.
int enc_forward_on(arp_enc* e, hipStream_t stream, const float* images_dev, int n, float* out_dev, const EncSeq& seq = {}, bool latency = false);
int enc_geometry(arp_enc* e, int* tokens, int* width, int* img_res, int* device);
int enc_seq_tokens(arp_enc* e, const EncSeq& seq, int* tokens);  // rows per sample of such a pass

// ONE instruction as a handle keeps it for its passes (model BC, InstructRL): L token ids followed by the visible-bit words, in HBM, and the words on the host.
struct EncText {
    DevBuf dev;
    std::vector<uint32_t> words;
    int L = 0;  // > 0: the instruction is set
    // tokens int32 [L], mask f32 [L] (> 0 = padded).  Refuses what a text pass of L tokens would refuse (the text weights, the mode, the length, an id outside
    // the vocabulary) and puts the position rows and the instruction on the device, synchronously; no pass in flight may still read the one it replaces.
    int set(arp_enc* e, const int32_t* tokens, const float* mask, int L);
    EncSeq seq() const { return EncSeq::text(L, 0, dev.as<int32_t>(), reinterpret_cast<const uint32_t*>(dev.as<int32_t>() + L), words.data()); }
};

// arp_op_gemm_site's "m3ae.*" instances (the encoder's own, in this unit)
int enc_op_gemm_site(const arp_gemm_site& d);
}  // namespace arp
