// CTC prefix beam search (Hannun et al. 2014), lexicon-free, with pyctcdecode's pruning knobs (token_min_logp, max_candidates,
// beam_prune_logp).  The semantics are written down in INTEGRATION.md ("CTC prefix beam search"); tests/ctc_beam_restatement.py
// restates them in float64.
//
// Two launches:
//   beam_prep_kernel: one wave per (utterance, frame) row, lanes over the vocabulary: the log-softmax normaliser and the
//     candidate list C_t (the up-to-K non-blank ids with the highest log probability >= token_min_logp, ties to the lower id).
//   beam_search_kernel: one workgroup per utterance loops over its frames; the hypotheses live in LDS in rank order.
// The normaliser and every score are fp64: the device then agrees with the float64 restatement to ~1e-12, far inside the
// smallest score gaps a real search meets (~1e-6 at W = 100, T = 249), so pruning and keep-W decisions are the same.
//
// Merging is exact.  Every hypothesis owns a node (parent node, token) of a per-utterance prefix tree in the workspace
// (node 0 = the empty prefix; the extension that survives frame t as rank q creates node 1 + t*W + q).  The extension of
// hypothesis i by c can only equal a live hypothesis j whose last token is c and whose prefix is the sequence of i: j is
// found through a hash of the token sequence (LDS open-addressing table of the live hypotheses) and then CHECKED by walking
// both parent chains in step until they meet or a token differs (the same sequence may own several nodes: a prefix that
// was pruned and found again gets a new node).
// Keep-W: a most-significant-digit radix select over the 96-bit composite (order-preserving bits of the score, then the
// complement of the origin key), 8 bits per pass, starting at the highest bit in which the surviving scores differ; the
// composites are unique, so the selected set has exactly W members.  The kept hypotheses are then ranked by counting.
//
// Language-model fusion (beam_search_kernel<true>, INTEGRATION.md "Language-model fusion"): the same search ranked by the
// fused score F = logaddexp(pb, pnb) + (lm + P), where lm sums the word terms of the completed words and P penalises a
// partial word that spells no prefix of a unigram.  Each hypothesis also carries its trie node, the code-point length of its
// partial word and its last LM_CTX word ids.  Per frame, the candidates' token kinds and code points are staged in LDS;
// each thread walks the trie for its unmerged character candidates (LM_WALK walks advance together, one probe per round)
// and scores the word a delimiter completes once (all n-gram probes of one lookup in flight together, ngram_lm.h).  The
// trie node each extension reaches is kept in LDS (x_node) for the ranking passes and the next frame's state.  After the
// last frame the hypotheses gain their end-of-utterance terms and are re-ranked by the final F.  beam_search_kernel<false>
// is the LM-free search, unchanged.
//
// Hotword boosting (beam_search_kernel<LM, true>, INTEGRATION.md "Hotword boosting"), with or without the LM: F gains
// weight * count(words) and the partial-word term R(p), the hotword bonus Q(p) where p is a prefix of a hotword unigram and
// otherwise the LM penalty P(p) (0 without the LM).  Each hypothesis also carries the hotword-trie node of p, its decided
// matches, its window of undecided words and its count (the window rule of hotword.h); the node each extension reaches is
// kept in LDS (x_hn), and the window step a delimiter takes is done once per thread (x_hc, x_hd, x_hwl, x_hw).
//
// Per-request hotwords (conformer_hip3_hotword_rows.h, INTEGRATION.md "Per-request hotwords"): LmParams<LM, true> may carry a
// table pointer and a weight per utterance; each workgroup resolves its own pair once before the frame loop (block-uniform, so
// the view stays in scalar registers) and everything above runs on it.  Null arrays: the launch-wide pair, as before.
//
// Timestamps (beam_search_kernel<LM, HW, true, true>, beam_commit_kernel<true>, INTEGRATION.md "Beam-search timestamps"): the
// resumable search also records, per created tree node, the absolute frame and the log-probability of its extension
// (TimesParams), the tracebacks return them beside the tokens and the commit carries them along (CommitTimes).
#include <float.h>
#include <type_traits>
#include "cfm_common.h"
#include "../../include/conformer_hip_commit.h"
#include "../../include/conformer_hip_times.h"
#include "conformer_hip3_hotword_rows.h"
#include "hotword.h"
#include "ngram_lm.h"

namespace {

constexpr int BEAM_MAX_W = 256;          // also the workgroup size of the search: thread i owns hypothesis i
constexpr int BEAM_MAX_K = 32;
constexpr int BEAM_TABLE = 512;          // hash slots (>= 2 W)
constexpr int BEAM_MAX_V = 1 << 23;      // origin keys rank * (V + 1) + token + 1 fit in 31 bits
constexpr int LM_TOK_CP = 8;             // code points of a candidate token staged in LDS (the rest is read from the tables)
constexpr int LM_WALK = 8;               // trie walks a thread advances together
constexpr double LN10 = 2.302585092994045684;

template <bool LM, bool HW = false> struct LmParams {};
template <> struct LmParams<true, false> {
    const void* tables;                  // cfm_ngram_lm_pack blob on the device
    double alpha, beta, unk_offset;
    int score_boundary;
    float* am_scores;
};
template <bool LM> struct LmParams<LM, true> {
    const void* tables;                  // cfm_ngram_lm_pack blob on the device (LM only)
    double alpha, beta, unk_offset;
    int score_boundary;
    float* am_scores;
    const void* hw_tables;               // cfm_hotword_pack blob on the device
    double hw_weight;
    // per-request hotwords (conformer_hip3_hotword_rows.h): (B) device arrays, the table and the weight of each utterance;
    // null: every utterance takes the pair above
    const void* const* hw_rows;
    const double* hw_row_weights;
};

// Resumable search (beam_search_kernel<LM, HW, true>, INTEGRATION.md "Streaming (resumable) search"): the state the one-shot
// kernel keeps in LDS between frames, saved per utterance in the stream buffer of cfm_ctc_beam_stream_*.  Hypotheses are
// stored in rank order; h_par and the hash table are rebuilt from the tree and the hashes when a step resumes.
template <bool ST> struct StreamParams {};
template <> struct StreamParams<true> {
    int* frames;                         // (B) frames consumed so far (absolute frame index of the next frame)
    int* nh;                             // (B) live hypotheses
    double *pb, *pnb, *s;                // (B, W)
    unsigned long long* hash;            // (B, W)
    int *node, *last, *len;              // (B, W)
    double* lm;                          // LM: (B, W) completed-word sum
    int *tn, *pl, *ctx;                  // LM: (B, W) trie node, partial length; (B, LM_CTX, W) context
    int *hn, *hd, *hwl, *hc;             // hotwords: (B, W)
    short* hw;                           // hotwords: (B, HW_WIN, W) window
    float* am_out;                       // interim acoustic scores (B, N) or null
    int t_max;                           // frames the tree has room for
    int finish;                          // 0: save the state and write the interim best; 1: end-of-utterance outputs
};

// Beam-search timestamps (beam_search_kernel<LM, HW, true, true>, INTEGRATION.md "Beam-search timestamps"): a caller-owned buffer
// beside the stream state.  Per utterance the absolute frame count since the utterance was opened (the stream state's own count
// becomes relative in commit mode), and per prefix-tree node the (frame, log-probability) of the extension that created it,
// parallel to BeamWs::nodes.  A stay keeps its node, so it keeps its record: the record of a token is its ENTRY on the lineage
// that survived.  The search adds one 8-byte global store per created node and no LDS.
template <bool TM> struct TimesParams {};
template <> struct TimesParams<true> {
    int64_t* count;                      // (B) frames consumed since the utterance was opened
    int2* rec;                           // (B, 1 + T*W) (frame, bits of the fp32 log-probability) per tree node
    int64_t* token_frames;               // (B, N, TO) beside `tokens`, padded with -1
    float* token_logp;                   // (B, N, TO) padded with -inf
};

// P(p): 0 for an empty partial word or one that spells a prefix of some unigram (node >= 0)
__device__ __forceinline__ double lm_pen(int node, int plen, double unk) {
    return (plen == 0 || node >= 0) ? 0.0 : unk * fmax(1.0, (double)plen / 6.0);
}

struct BeamWs {
    double* lse;      // (B*T) log-sum-exp of each logits row
    int* ncand;       // (B*T) |C_t|
    int* ctok;        // (B*T, K) candidate ids, best first
    double* clp;      // (B*T, K) their log probabilities
    int2* nodes;      // (B, 1 + T*W) prefix-tree nodes (parent, token)
};

inline size_t beam_align(size_t x) { return (x + 255) & ~size_t(255); }

inline size_t beam_carve(int B, int T, int W, int K, char* base, BeamWs* ws) {
    const size_t rows = (size_t)B * T;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += beam_align(bytes); return p; };
    char* lse = take(rows * sizeof(double));
    char* ncand = take(rows * sizeof(int));
    char* ctok = take(rows * K * sizeof(int));
    char* clp = take(rows * K * sizeof(double));
    char* nodes = take((size_t)B * (1 + (size_t)T * W) * sizeof(int2));
    if (ws) *ws = BeamWs{(double*)lse, (int*)ncand, (int*)ctok, (double*)clp, (int2*)nodes};
    return off;
}

// the stream buffer: the one-shot workspace for T_max frames (candidate rows of one chunk, the prefix tree of the whole
// stream), then the saved search state
inline size_t stream_carve(int B, int Tm, int W, int K, bool lm, bool hw, char* base, BeamWs* ws, StreamParams<true>* sp) {
    size_t off = beam_carve(B, Tm, W, K, base, ws);
    const size_t bw = (size_t)B * W;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += beam_align(bytes); return p; };
    StreamParams<true> p{};
    p.frames = (int*)take(B * sizeof(int));
    p.nh = (int*)take(B * sizeof(int));
    p.pb = (double*)take(bw * sizeof(double));
    p.pnb = (double*)take(bw * sizeof(double));
    p.s = (double*)take(bw * sizeof(double));
    p.hash = (unsigned long long*)take(bw * sizeof(unsigned long long));
    p.node = (int*)take(bw * sizeof(int));
    p.last = (int*)take(bw * sizeof(int));
    p.len = (int*)take(bw * sizeof(int));
    if (lm) {
        p.lm = (double*)take(bw * sizeof(double));
        p.tn = (int*)take(bw * sizeof(int));
        p.pl = (int*)take(bw * sizeof(int));
        p.ctx = (int*)take(bw * LM_CTX * sizeof(int));
    }
    if (hw) {
        p.hn = (int*)take(bw * sizeof(int));
        p.hd = (int*)take(bw * sizeof(int));
        p.hwl = (int*)take(bw * sizeof(int));
        p.hc = (int*)take(bw * sizeof(int));
        p.hw = (short*)take(bw * HW_WIN * sizeof(short));
    }
    p.t_max = Tm;
    if (sp) *sp = p;
    return off;
}

__device__ __forceinline__ int beam_frames(const int64_t* lengths, int b, int T) {
    return lengths ? (int)min((int64_t)T, max((int64_t)0, lengths[b])) : T;
}

// (x, c) precedes (bx, bc) in candidate order: higher logit first, ties to the lower id; bc == INT_MAX is "none"
__device__ __forceinline__ bool cand_before(float x, int c, float bx, int bc) {
    return bc == INT_MAX || x > bx || (x == bx && c < bc);
}

__global__ __launch_bounds__(256) void beam_prep_kernel(const float* __restrict__ logits, const int64_t* __restrict__ lengths,
                                                        BeamWs ws, int B, int T, int V, int blank, int K, double token_min_logp) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)B * T) return;
    const int b = (int)(row / T), t = (int)(row % T);
    if (t >= beam_frames(lengths, b, T)) return;                // rows the search does not consume
    const float* r = logits + row * V;
    float m = -INFINITY;
    for (int c = lane; c < V; c += 64) m = fmaxf(m, r[c]);
    m = wave_max(m);
    double sum = 0.0;
    for (int c = lane; c < V; c += 64) sum += exp((double)r[c] - (double)m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const double lse = (double)m + log(sum);
    // C_t by K rounds of a wave arg-max over the entries that follow the previous pick in candidate order.  lp = x - lse is
    // monotone in x, so the order of the fp32 logits is the order of the log probabilities.
    float px = INFINITY;
    int pc = -1, cnt = 0;
    for (int k = 0; k < K; ++k) {
        float bx = -INFINITY;
        int bc = INT_MAX;
        for (int c = lane; c < V; c += 64) {
            const float x = r[c];
            if (c == blank || !((double)x - lse >= token_min_logp)) continue;          // also drops NaN
            if (!(x < px || (x == px && c > pc))) continue;                           // already picked
            if (cand_before(x, c, bx, bc)) { bx = x; bc = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ox = __shfl_xor(bx, o, 64);
            const int oc = __shfl_xor(bc, o, 64);
            if (oc != INT_MAX && cand_before(ox, oc, bx, bc)) { bx = ox; bc = oc; }
        }
        if (bc == INT_MAX) break;                                  // wave-uniform after the butterfly
        if (lane == 0) {
            ws.ctok[row * K + k] = bc;
            ws.clp[row * K + k] = (double)bx - lse;
        }
        px = bx; pc = bc; ++cnt;
    }
    if (lane == 0) {
        ws.lse[row] = lse;
        ws.ncand[row] = cnt;
    }
}

__device__ __forceinline__ double lae(double a, double b) {            // log(exp(a) + exp(b))
    const double m = a > b ? a : b;
    if (m == -INFINITY) return -INFINITY;
    return m + log1p(exp(-fabs(a - b)));
}

// order-preserving unsigned image of a double (larger double -> larger image; NaN never reaches it)
__device__ __forceinline__ unsigned long long ord64(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
}

__device__ __forceinline__ unsigned long long seq_hash(unsigned long long h, int c) {
    unsigned long long z = h + (unsigned long long)(c + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr unsigned long long ROOT_HASH = 0x243F6A8885A308D3ull;

// nodes a and b stand for sequences of the same length: are the sequences equal?
__device__ bool same_sequence(const int2* nd, int a, int b, int len) {
    for (int step = 0; step <= len; ++step) {
        if (a == b) return true;
        if (a <= 0 || b <= 0) return false;
        const int2 na = nd[a], nb = nd[b];
        if (na.y != nb.y) return false;
        a = na.x; b = nb.x;
    }
    return false;
}

typedef unsigned __int128 u128;

template <bool LM, bool HW, bool ST = false, bool TM = false>
__global__ __launch_bounds__(BEAM_MAX_W) void beam_search_kernel(
        const float* __restrict__ logits, const int64_t* __restrict__ lengths, BeamWs ws, int T, int V, int blank, int W,
        int K, double prune, int N, int64_t* __restrict__ tokens, int64_t* __restrict__ counts, float* __restrict__ scores,
        int64_t* __restrict__ num_hyps, LmParams<LM, HW> lp, StreamParams<ST> sp = {}, TimesParams<TM> tp = {}) {
    static_assert(ST || !TM, "timestamps are recorded by the resumable search");
    // hypotheses in rank order, double-buffered across frames
    __shared__ double h_pb[2][BEAM_MAX_W], h_pnb[2][BEAM_MAX_W], h_s[2][BEAM_MAX_W];
    __shared__ unsigned long long h_hash[2][BEAM_MAX_W];
    __shared__ int h_node[2][BEAM_MAX_W], h_par[2][BEAM_MAX_W], h_last[2][BEAM_MAX_W], h_len[2][BEAM_MAX_W];
    __shared__ double m_val[BEAM_MAX_W];              // extension merged into hypothesis j: its value and origin key
    __shared__ unsigned m_key[BEAM_MAX_W];
    __shared__ int c_tok[BEAM_MAX_K];
    __shared__ double c_lp[BEAM_MAX_K];
    __shared__ int table[BEAM_TABLE];
    __shared__ unsigned hist[2][256];
    __shared__ double red_best[4];
    __shared__ int red_cnt[4];
    __shared__ unsigned long long red_min[4];
    __shared__ int sel_d, sel_need, sel_done, n_kept;
    // the kept candidates before ranking
    __shared__ unsigned long long l_ord[BEAM_MAX_W];
    __shared__ unsigned l_low[BEAM_MAX_W];
    __shared__ int l_item[BEAM_MAX_W];
    __shared__ double l_pb[BEAM_MAX_W], l_pnb[BEAM_MAX_W], l_s[BEAM_MAX_W];
    // language-model state of the hypotheses (double-buffered like the rest), this frame's candidate tokens, and per
    // thread: the word term its delimiters add, the word id they push, the trie node each candidate reaches
    constexpr int LW = LM ? BEAM_MAX_W : 1, LK = LM ? BEAM_MAX_K : 1, TK = (LM || HW) ? BEAM_MAX_K : 1;
    __shared__ double h_lm[2][LW], x_term[LW];
    __shared__ int h_tn[2][LW], h_pl[2][LW], h_ctx[2][LM_CTX][LW], x_wid[LW], x_node[LK][LW];
    __shared__ int c_kind[TK], c_len[TK], c_off[TK], c_cp[TK][LM_TOK_CP];
    // hotword state of the hypotheses (trie node of p, decided matches, window length, count, window), per thread the state
    // after the word its delimiters complete, and the hotword-trie node each candidate reaches
    constexpr int HWW = HW ? BEAM_MAX_W : 1, HK = HW ? BEAM_MAX_K : 1;
    __shared__ int h_hn[2][HWW], h_hd[2][HWW], h_hwl[2][HWW], h_hc[2][HWW], x_hd[HWW], x_hwl[HWW], x_hc[HWW], x_hn[HK][HWW];
    __shared__ short h_hw[2][HW_WIN][HWW], x_hw[HW_WIN][HWW];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // ST: T is the chunk's frame count; the tree and the outputs span the stream's TO = t_max frames, and frame t of the
    // chunk is frame t0 + t of the utterance
    int n = beam_frames(lengths, b, T), t0 = 0;
    int TO = T;
    if constexpr (ST) {
        TO = sp.t_max;
        t0 = sp.frames[b];
        n = min(n, TO - t0);                                 // (the host refuses a chunk that could pass t_max)
    }
    int2* nd = ws.nodes + (int64_t)b * (1 + (int64_t)TO * W);
    // TM: the records of this utterance's nodes and the absolute index of the chunk's frame 0
    [[maybe_unused]] int2* tr = nullptr;
    [[maybe_unused]] int64_t a0 = 0;
    if constexpr (TM) {
        tr = tp.rec + (int64_t)b * (1 + (int64_t)TO * W);
        a0 = tp.count[b];
    }
    const unsigned V1 = (unsigned)V + 1u;
    [[maybe_unused]] LmView lmv;
    if constexpr (LM) lmv = lm_view(lp.tables);
    [[maybe_unused]] HwView hwv;
    [[maybe_unused]] const int32_t* tok_cp = nullptr;      // code points of the tokens (LM blob, else hotword blob)
    [[maybe_unused]] double hww = 0.0;                     // this utterance's hotword weight
    if constexpr (HW) {
        // the table and the weight of this utterance: b is blockIdx.x, so both loads and the view are workgroup-uniform
        const void* hwt = lp.hw_tables;
        hww = lp.hw_weight;
        // (a pointer loaded from memory is a generic one to the compiler and every table read would become a flat load; the
        // tables are device memory, so it goes through the global address space like the launch-wide kernel argument)
        typedef __attribute__((address_space(1))) const char* global_table;
        if (lp.hw_rows) hwt = (const void*)(global_table)(uintptr_t)lp.hw_rows[b];
        if (lp.hw_row_weights) hww = lp.hw_row_weights[b];
        hwv = hw_view(hwt);
        if constexpr (LM) tok_cp = lmv.tok_cp;
        else tok_cp = hwv.tok_cp;
    }

    int cur = 0, nh = 1;
    for (int i = tid; i < BEAM_TABLE; i += BEAM_MAX_W) table[i] = -1;
    if constexpr (ST) {
        // resume: the saved hypotheses in rank order, their parents from the tree, then the hash table (any insertion
        // order gives the same merges: live hypotheses are distinct sequences and every hit is checked against the tree)
        nh = sp.nh[b];
        const int64_t o = (int64_t)b * W + tid;
        if (tid < nh) {
            h_pb[0][tid] = sp.pb[o]; h_pnb[0][tid] = sp.pnb[o]; h_s[0][tid] = sp.s[o]; h_hash[0][tid] = sp.hash[o];
            const int node = sp.node[o];
            h_node[0][tid] = node; h_par[0][tid] = node > 0 ? nd[node].x : -1;
            h_last[0][tid] = sp.last[o]; h_len[0][tid] = sp.len[o];
            if constexpr (LM) {
                h_lm[0][tid] = sp.lm[o]; h_tn[0][tid] = sp.tn[o]; h_pl[0][tid] = sp.pl[o];
                for (int i = 0; i < LM_CTX; ++i) h_ctx[0][i][tid] = sp.ctx[((int64_t)b * LM_CTX + i) * W + tid];
            }
            if constexpr (HW) {
                h_hn[0][tid] = sp.hn[o]; h_hd[0][tid] = sp.hd[o]; h_hwl[0][tid] = sp.hwl[o]; h_hc[0][tid] = sp.hc[o];
                for (int u = 0; u < HW_WIN; ++u) h_hw[0][u][tid] = sp.hw[((int64_t)b * HW_WIN + u) * W + tid];
            }
        }
        __syncthreads();
        if (tid < nh) {
            int slot = (int)(h_hash[0][tid] & (BEAM_TABLE - 1));
            for (int p = 0; p < BEAM_TABLE && atomicCAS(&table[slot], -1, tid) != -1; ++p) slot = (slot + 1) & (BEAM_TABLE - 1);
        }
        __syncthreads();
    } else {
        if (tid == 0) {
            h_pb[0][0] = 0.0; h_pnb[0][0] = -INFINITY; h_s[0][0] = 0.0;
            h_hash[0][0] = ROOT_HASH; h_node[0][0] = 0; h_par[0][0] = -1; h_last[0][0] = -1; h_len[0][0] = 0;
            nd[0] = make_int2(-1, -1);
            if constexpr (LM) {
                h_lm[0][0] = 0.0; h_tn[0][0] = 0; h_pl[0][0] = 0;
                for (int i = 0; i < LM_CTX; ++i) h_ctx[0][i][0] = -1;
                if (lp.score_boundary) h_ctx[0][LM_CTX - 1][0] = lmv.bos;
            }
            if constexpr (HW) {
                h_hn[0][0] = 0; h_hd[0][0] = 0; h_hwl[0][0] = 0; h_hc[0][0] = 0;
                for (int u = 0; u < HW_WIN; ++u) h_hw[0][u][0] = -1;
            }
        }
        __syncthreads();
        if (tid == 0) table[ROOT_HASH & (BEAM_TABLE - 1)] = 0;
    }

    for (int t = 0; t < n; ++t) {
        const int64_t row = (int64_t)b * T + t;
        const int nc = ws.ncand[row];
        const double lse = ws.lse[row];
        const float* lrow = logits + row * V;
        // ---- A: this frame's candidates; own hypothesis; stays
        if (tid < nc) { c_tok[tid] = ws.ctok[row * K + tid]; c_lp[tid] = ws.clp[row * K + tid]; }
        if constexpr (LM) {
            if (tid < nc) {
                const int c = ws.ctok[row * K + tid];
                int kind = LM_TOK_SKIP, o = 0, l = 0;
                if (c < lmv.V) { kind = lmv.tok_kind[c]; o = lmv.tok_off[c]; l = lmv.tok_off[c + 1] - o; }
                if (kind != LM_TOK_CHARS) l = 0;
                c_kind[tid] = kind; c_off[tid] = o; c_len[tid] = l;
                for (int q = 0; q < min(l, LM_TOK_CP); ++q) c_cp[tid][q] = lmv.tok_cp[o + q];
            }
        } else if constexpr (HW) {
            if (tid < nc) {
                const int c = ws.ctok[row * K + tid];
                int kind = LM_TOK_SKIP, o = 0, l = 0;
                if (c < hwv.V) { kind = hwv.tok_kind[c]; o = hwv.tok_off[c]; l = hwv.tok_off[c + 1] - o; }
                if (kind != LM_TOK_CHARS) l = 0;
                c_kind[tid] = kind; c_off[tid] = o; c_len[tid] = l;
                for (int q = 0; q < min(l, LM_TOK_CP); ++q) c_cp[tid][q] = hwv.tok_cp[o + q];
            }
        }
        hist[0][tid] = 0u;
        if (tid == 0) n_kept = 0;
        const bool own = tid < nh;
        double pb = 0, pnb = 0, s = 0, st_pb = -INFINITY, st_pnb = -INFINITY;
        int last = -1, len = 0, node = 0;
        unsigned long long hash = 0;
        // LM state of the own hypothesis: completed-word sum, trie node, partial length, context; lm + P; the word term
        [[maybe_unused]] double lm = 0, lmp = 0, term = 0;
        [[maybe_unused]] int tn = 0, pl = 0;
        [[maybe_unused]] int ctx[LM_CTX];
        // hotword state of the own hypothesis: trie node of p, count; weight * count, and after a delimiter's word
        [[maybe_unused]] int hn = 0, hc = 0;
        [[maybe_unused]] double hwc = 0, xhwc = 0;
        if (own) {
            pb = h_pb[cur][tid]; pnb = h_pnb[cur][tid]; s = h_s[cur][tid];
            last = h_last[cur][tid]; len = h_len[cur][tid]; node = h_node[cur][tid]; hash = h_hash[cur][tid];
            if constexpr (LM) {
                lm = h_lm[cur][tid]; tn = h_tn[cur][tid]; pl = h_pl[cur][tid];
                for (int i = 0; i < LM_CTX; ++i) ctx[i] = h_ctx[cur][i][tid];
                lmp = lm + lm_pen(tn, pl, lp.unk_offset);
            }
            if constexpr (HW) {
                hn = h_hn[cur][tid]; hc = h_hc[cur][tid];
                hwc = hww * (double)hc;
                double r;
                if constexpr (LM) r = hn >= 0 ? hw_bonus(hwv, hn, hww) : lm_pen(tn, pl, lp.unk_offset);
                else r = hw_bonus(hwv, hn, hww);
                lmp = (lm + hwc) + r;
            }
            st_pb = s + ((double)lrow[blank] - lse);
            st_pnb = last >= 0 ? pnb + ((double)lrow[last] - lse) : -INFINITY;
            m_val[tid] = -INFINITY;
            m_key[tid] = 0xFFFFFFFFu;
        }
        __syncthreads();
        // ---- B: extensions that equal a live hypothesis fold into its stay
        unsigned mask = 0;
        if (own) {
            for (int k = 0; k < nc; ++k) {
                const int c = c_tok[k];
                const unsigned long long target = seq_hash(hash, c);
                for (int p = 0, slot = (int)(target & (BEAM_TABLE - 1)); p < BEAM_TABLE; ++p, slot = (slot + 1) & (BEAM_TABLE - 1)) {
                    const int j = table[slot];
                    if (j < 0) break;
                    if (h_hash[cur][j] == target && h_last[cur][j] == c && h_len[cur][j] == len + 1 &&
                        same_sequence(nd, h_par[cur][j], node, len)) {
                        mask |= 1u << k;
                        m_val[j] = (c == last ? pb : s) + c_lp[k];
                        m_key[j] = (unsigned)tid * V1 + (unsigned)c + 1u;
                        break;
                    }
                }
            }
            if constexpr (LM) {
                // the word a delimiter completes (the same for every delimiter candidate)
                bool delim = false;
                for (int k = 0; k < nc; ++k) delim |= !((mask >> k) & 1u) && c_kind[k] == LM_TOK_DELIM;
                if (delim && pl > 0) {
                    const int wd = tn >= 0 ? lmv.node_word[tn] : -1;
                    const int w = wd >= 0 ? wd : lmv.unk;
                    term = lp.alpha * LN10 * (lm_cond_log10(lmv, ctx, w) + (wd >= 0 ? 0.0 : lp.unk_offset)) + lp.beta;
                    x_term[tid] = term;
                    x_wid[tid] = w;
                }
                // trie walks of the character candidates, LM_WALK at a time
                auto cp_at = [&](int k, int q) { return q < LM_TOK_CP ? c_cp[k][q] : lmv.tok_cp[c_off[k] + q]; };
                for (int k0 = 0; k0 < nc; k0 += LM_WALK) {
                    int wn[LM_WALK], wq[LM_WALK];
                    unsigned wsl[LM_WALK];
                    bool wa[LM_WALK];
#pragma unroll
                    for (int u = 0; u < LM_WALK; ++u) {
                        const int k = k0 + u;
                        wn[u] = tn; wq[u] = 0; wsl[u] = 0u;
                        wa[u] = k < nc && tn >= 0 && !((mask >> k) & 1u) && c_len[k] > 0;
                        if (wa[u]) wsl[u] = (unsigned)trie_hash(tn, cp_at(k, 0)) & lmv.trie_mask;
                    }
                    for (;;) {
                        bool any = false;
#pragma unroll
                        for (int u = 0; u < LM_WALK; ++u) any |= wa[u];
                        if (!any) break;
                        int4 e[LM_WALK];
#pragma unroll
                        for (int u = 0; u < LM_WALK; ++u)
                            if (wa[u]) e[u] = lmv.trie[wsl[u]];
#pragma unroll
                        for (int u = 0; u < LM_WALK; ++u) {
                            if (!wa[u]) continue;
                            const int k = k0 + u, cp = cp_at(k, wq[u]);
                            if (e[u].x == -1) {                                  // no such edge: no unigram has this prefix
                                wn[u] = -1; wa[u] = false;
                            } else if (e[u].x == wn[u] && e[u].y == cp) {
                                wn[u] = e[u].z;
                                if (++wq[u] == c_len[k]) wa[u] = false;
                                else wsl[u] = (unsigned)trie_hash(wn[u], cp_at(k, wq[u])) & lmv.trie_mask;
                            } else {
                                wsl[u] = (wsl[u] + 1u) & lmv.trie_mask;
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < LM_WALK; ++u)
                        if (k0 + u < nc) x_node[k0 + u][tid] = wn[u];
                }
            }
            if constexpr (HW) {
                // the window step of the word a delimiter completes (the same for every delimiter candidate)
                bool delim = false;
                for (int k = 0; k < nc; ++k) delim |= !((mask >> k) & 1u) && c_kind[k] == LM_TOK_DELIM;
                if (delim && hn != 0) {
                    int ids[HW_WIN];
#pragma unroll
                    for (int u = 0; u < HW_WIN; ++u) ids[u] = h_hw[cur][u][tid];
                    int wl = h_hwl[cur][tid], dec = h_hd[cur][tid];
                    const int c = hw_push(hwv, ids, wl, dec, hn > 0 ? hwv.cnode[hn].x : -1);
                    x_hc[tid] = c; x_hd[tid] = dec; x_hwl[tid] = wl;
#pragma unroll
                    for (int u = 0; u < HW_WIN; ++u) x_hw[u][tid] = (short)ids[u];
                    xhwc = hww * (double)c;
                }
                // hotword-trie walks of the character candidates, LM_WALK at a time
                auto cp_at = [&](int k, int q) { return q < LM_TOK_CP ? c_cp[k][q] : tok_cp[c_off[k] + q]; };
                for (int k0 = 0; k0 < nc; k0 += LM_WALK) {
                    int wn[LM_WALK], wq[LM_WALK];
                    unsigned wsl[LM_WALK];
                    bool wa[LM_WALK];
#pragma unroll
                    for (int u = 0; u < LM_WALK; ++u) {
                        const int k = k0 + u;
                        wn[u] = hn; wq[u] = 0; wsl[u] = 0u;
                        wa[u] = k < nc && hn >= 0 && !((mask >> k) & 1u) && c_len[k] > 0;
                        if (wa[u]) wsl[u] = (unsigned)trie_hash(hn, cp_at(k, 0)) & hwv.ctrie_mask;
                    }
                    for (;;) {
                        bool any = false;
#pragma unroll
                        for (int u = 0; u < LM_WALK; ++u) any |= wa[u];
                        if (!any) break;
                        int4 e[LM_WALK];
#pragma unroll
                        for (int u = 0; u < LM_WALK; ++u)
                            if (wa[u]) e[u] = hwv.ctrie[wsl[u]];
#pragma unroll
                        for (int u = 0; u < LM_WALK; ++u) {
                            if (!wa[u]) continue;
                            const int k = k0 + u, cp = cp_at(k, wq[u]);
                            if (e[u].x == -1) {                                  // no such edge: no hotword unigram has this prefix
                                wn[u] = -1; wa[u] = false;
                            } else if (e[u].x == wn[u] && e[u].y == cp) {
                                wn[u] = e[u].z;
                                if (++wq[u] == c_len[k]) wa[u] = false;
                                else wsl[u] = (unsigned)trie_hash(wn[u], cp_at(k, wq[u])) & hwv.ctrie_mask;
                            } else {
                                wsl[u] = (wsl[u] + 1u) & hwv.ctrie_mask;
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < LM_WALK; ++u)
                        if (k0 + u < nc) x_hn[k0 + u][tid] = wn[u];
                }
            }
        }
        __syncthreads();
        // lm + P after the own hypothesis is extended by candidate k (LM only)
        [[maybe_unused]] auto ext_lmp = [&](int k) -> double {
            if constexpr (HW) {
                const int kind = c_kind[k];
                if (kind == LM_TOK_CHARS) {
                    const int xn = x_hn[k][tid];
                    double r;
                    if constexpr (LM) r = xn >= 0 ? hw_bonus(hwv, xn, hww) : lm_pen(x_node[k][tid], pl + c_len[k], lp.unk_offset);
                    else r = hw_bonus(hwv, xn, hww);
                    return (lm + hwc) + r;
                }
                if (kind == LM_TOK_DELIM && hn != 0) return ((lm + term) + xhwc) + 0.0;
                return lmp;
            } else if constexpr (LM) {
                const int kind = c_kind[k];
                if (kind == LM_TOK_CHARS) return lm + lm_pen(x_node[k][tid], pl + c_len[k], lp.unk_offset);
                if (kind == LM_TOK_DELIM && pl > 0) return (lm + term) + 0.0;
                return lmp;
            } else {
                return 0.0;
            }
        };
        // ---- C: stay scores and the best candidate score
        for (int i = tid; i < BEAM_TABLE; i += BEAM_MAX_W) table[i] = -1;
        double st_score = -INFINITY, best = -INFINITY;
        [[maybe_unused]] double st_am = -INFINITY;
        unsigned st_key = 0;
        if (own) {
            st_pnb = lae(st_pnb, m_val[tid]);
            st_score = lae(st_pb, st_pnb);
            if constexpr (LM || HW) { st_am = st_score; st_score = st_am + lmp; }         // stays rank by the fused score
            st_key = min((unsigned)tid * V1, m_key[tid]);
            best = st_score;
            for (int k = 0; k < nc; ++k) {
                if ((mask >> k) & 1u) continue;
                double e = (c_tok[k] == last ? pb : s) + c_lp[k];
                if constexpr (LM || HW) e = e + ext_lmp(k);
                if (e > best) best = e;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const double x = __shfl_xor(best, o, 64); if (x > best) best = x; }
        if (lane == 0) red_best[wv] = best;
        __syncthreads();
        best = fmax(fmax(red_best[0], red_best[1]), fmax(red_best[2], red_best[3]));
        const double thr = best + prune;
        // ---- D: survivors (score >= best + prune): count, lowest score
        int cnt = 0;
        unsigned long long omin = ~0ull;
        if (own) {
            if (st_score >= thr) { ++cnt; omin = ord64(st_score); }
            for (int k = 0; k < nc; ++k) {
                if ((mask >> k) & 1u) continue;
                double e = (c_tok[k] == last ? pb : s) + c_lp[k];
                if constexpr (LM || HW) e = e + ext_lmp(k);
                if (e >= thr) { ++cnt; omin = min(omin, ord64(e)); }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cnt += __shfl_xor(cnt, o, 64);
            omin = min(omin, (unsigned long long)__shfl_xor(omin, o, 64));
        }
        if (lane == 0) { red_cnt[wv] = cnt; red_min[wv] = omin; }
        __syncthreads();
        const int S = red_cnt[0] + red_cnt[1] + red_cnt[2] + red_cnt[3];
        // ---- keep-W: radix select of the W largest composites (only when more than W survive)
        int pos = 0;
        u128 prefix = 0;
        if (S > W) {
            const unsigned long long diff = ord64(best) ^ min(min(red_min[0], red_min[1]), min(red_min[2], red_min[3]));
            const int top = diff ? 32 + 64 - __clzll((long long)diff) : 32;
            pos = (top + 7) & ~7;
            prefix = ((u128)ord64(best) << 32) >> pos;                  // the bits every survivor shares
            int need = W;
            for (int pass = 0; pos > 0; ++pass) {
                const int buf = pass & 1;
                hist[buf ^ 1][tid] = 0u;
                if (own) {
                    for (int k = -1; k < nc; ++k) {
                        double e;
                        unsigned key;
                        if (k < 0) { e = st_score; key = st_key; }
                        else {
                            if ((mask >> k) & 1u) continue;
                            e = (c_tok[k] == last ? pb : s) + c_lp[k];
                            if constexpr (LM || HW) e = e + ext_lmp(k);
                            key = (unsigned)tid * V1 + (unsigned)c_tok[k] + 1u;
                        }
                        if (!(e >= thr)) continue;
                        const u128 comp = ((u128)ord64(e) << 32) | (u128)(0xFFFFFFFFu - key);
                        if ((comp >> pos) == prefix) atomicAdd(&hist[buf][(unsigned)(comp >> (pos - 8)) & 255u], 1u);
                    }
                }
                __syncthreads();
                if (wv == 0) {
                    unsigned h[4], sum = 0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) { h[q] = hist[buf][4 * lane + q]; sum += h[q]; }
                    unsigned suf = sum;                                   // bins of lanes >= lane
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const unsigned x = __shfl_down(suf, o, 64);
                        if (lane + o < 64) suf += x;
                    }
                    unsigned above = suf - sum;
#pragma unroll
                    for (int q = 3; q >= 0; --q) {
                        if (above < (unsigned)need && above + h[q] >= (unsigned)need) {
                            sel_d = 4 * lane + q;
                            sel_need = need - (int)above;
                            sel_done = h[q] == (unsigned)(need - (int)above);
                        }
                        above += h[q];
                    }
                }
                __syncthreads();
                prefix = (prefix << 8) | (u128)(unsigned)sel_d;
                pos -= 8;
                need = sel_need;
                if (sel_done) break;
            }
        }
        // ---- E: compaction of the kept candidates
        if (own) {
            for (int k = -1; k < nc; ++k) {
                double e, ipb, ipnb;
                [[maybe_unused]] double am;                          // LM: the acoustic score beside the fused e
                unsigned key;
                if (k < 0) {
                    e = st_score; key = st_key; ipb = st_pb; ipnb = st_pnb;
                    if constexpr (LM || HW) am = st_am;
                } else {
                    if ((mask >> k) & 1u) continue;
                    e = (c_tok[k] == last ? pb : s) + c_lp[k];
                    key = (unsigned)tid * V1 + (unsigned)c_tok[k] + 1u;
                    ipb = -INFINITY; ipnb = e;
                    if constexpr (LM || HW) { am = e; e = e + ext_lmp(k); }
                }
                if (!(e >= thr)) continue;
                const u128 comp = ((u128)ord64(e) << 32) | (u128)(0xFFFFFFFFu - key);
                if (S > W && (comp >> pos) < prefix) continue;
                const int slot = atomicAdd(&n_kept, 1);
                if (slot < W) {
                    l_ord[slot] = ord64(e); l_low[slot] = 0xFFFFFFFFu - key; l_item[slot] = tid * 64 + (k + 1);
                    l_pb[slot] = ipb; l_pnb[slot] = ipnb;
                    if constexpr (LM || HW) l_s[slot] = am;
                    else l_s[slot] = e;
                }
            }
        }
        __syncthreads();
        // ---- F: rank the kept hypotheses by counting, write the next frame's state, rebuild the table
        const int M = min(n_kept, W);
        const int nxt = cur ^ 1;
        if (tid < M) {
            const unsigned long long o = l_ord[tid];
            const unsigned lo = l_low[tid];
            int q = 0;
            for (int j = 0; j < M; ++j) q += (l_ord[j] > o) || (l_ord[j] == o && l_low[j] > lo);
            const int i = l_item[tid] >> 6, k = (l_item[tid] & 63) - 1;
            h_pb[nxt][q] = l_pb[tid]; h_pnb[nxt][q] = l_pnb[tid]; h_s[nxt][q] = l_s[tid];
            unsigned long long qh;
            if (k < 0) {
                qh = h_hash[cur][i];
                h_node[nxt][q] = h_node[cur][i]; h_par[nxt][q] = h_par[cur][i]; h_last[nxt][q] = h_last[cur][i];
                h_len[nxt][q] = h_len[cur][i];
            } else {
                const int c = c_tok[k], id = 1 + (t0 + t) * W + q;
                nd[id] = make_int2(h_node[cur][i], c);
                if constexpr (TM) tr[id] = make_int2((int)(a0 + t), __float_as_int((float)c_lp[k]));
                qh = seq_hash(h_hash[cur][i], c);
                h_node[nxt][q] = id; h_par[nxt][q] = h_node[cur][i]; h_last[nxt][q] = c; h_len[nxt][q] = h_len[cur][i] + 1;
            }
            h_hash[nxt][q] = qh;
            if constexpr (LM) {
                double nlm = h_lm[cur][i];
                int ntn = h_tn[cur][i], npl = h_pl[cur][i], sh = 0;
                if (k >= 0) {
                    const int kind = c_kind[k];
                    if (kind == LM_TOK_CHARS) { ntn = x_node[k][i]; npl += c_len[k]; }
                    else if (kind == LM_TOK_DELIM && npl > 0) { nlm = (nlm + x_term[i]) + 0.0; ntn = 0; npl = 0; sh = 1; }
                }
                h_lm[nxt][q] = nlm; h_tn[nxt][q] = ntn; h_pl[nxt][q] = npl;
                for (int u = 0; u < LM_CTX; ++u)
                    h_ctx[nxt][u][q] = u + sh < LM_CTX ? h_ctx[cur][u + sh][i] : x_wid[i];
            }
            if constexpr (HW) {
                int nhn = h_hn[cur][i], nhd = h_hd[cur][i], nhl = h_hwl[cur][i], nhc = h_hc[cur][i];
                bool word = false;
                if (k >= 0) {
                    const int kind = c_kind[k];
                    if (kind == LM_TOK_CHARS) nhn = x_hn[k][i];
                    else if (kind == LM_TOK_DELIM && nhn != 0) { nhn = 0; nhd = x_hd[i]; nhl = x_hwl[i]; nhc = x_hc[i]; word = true; }
                }
                h_hn[nxt][q] = nhn; h_hd[nxt][q] = nhd; h_hwl[nxt][q] = nhl; h_hc[nxt][q] = nhc;
                for (int u = 0; u < HW_WIN; ++u) h_hw[nxt][u][q] = word ? x_hw[u][i] : h_hw[cur][u][i];
            }
            int slot = (int)(qh & (BEAM_TABLE - 1));
            for (int p = 0; p < BEAM_TABLE && atomicCAS(&table[slot], -1, q) != -1; ++p) slot = (slot + 1) & (BEAM_TABLE - 1);
        }
        __syncthreads();
        cur = nxt;
        nh = M;
    }

    if constexpr (ST) {
        if (!sp.finish) {
            // ---- save the state in rank order; write the interim best: the hypotheses as they rank now, with F without the
            // end-of-utterance terms (the fused score they were ranked by)
            const int64_t o = (int64_t)b * W + tid;
            double f = -INFINITY;
            if (tid < nh) {
                sp.pb[o] = h_pb[cur][tid]; sp.pnb[o] = h_pnb[cur][tid]; sp.s[o] = h_s[cur][tid]; sp.hash[o] = h_hash[cur][tid];
                sp.node[o] = h_node[cur][tid]; sp.last[o] = h_last[cur][tid]; sp.len[o] = h_len[cur][tid];
                [[maybe_unused]] double lm = 0.0, lmp = 0.0;
                if constexpr (LM) {
                    lm = h_lm[cur][tid];
                    sp.lm[o] = lm; sp.tn[o] = h_tn[cur][tid]; sp.pl[o] = h_pl[cur][tid];
                    for (int i = 0; i < LM_CTX; ++i) sp.ctx[((int64_t)b * LM_CTX + i) * W + tid] = h_ctx[cur][i][tid];
                    lmp = lm + lm_pen(h_tn[cur][tid], h_pl[cur][tid], lp.unk_offset);
                }
                if constexpr (HW) {
                    const int hn = h_hn[cur][tid], hc = h_hc[cur][tid];
                    sp.hn[o] = hn; sp.hd[o] = h_hd[cur][tid]; sp.hwl[o] = h_hwl[cur][tid]; sp.hc[o] = hc;
                    for (int u = 0; u < HW_WIN; ++u) sp.hw[((int64_t)b * HW_WIN + u) * W + tid] = h_hw[cur][u][tid];
                    double r;
                    if constexpr (LM) r = hn >= 0 ? hw_bonus(hwv, hn, hww) : lm_pen(h_tn[cur][tid], h_pl[cur][tid], lp.unk_offset);
                    else r = hw_bonus(hwv, hn, hww);
                    lmp = (lm + hww * (double)hc) + r;
                }
                f = h_s[cur][tid];
                if constexpr (LM || HW) f = f + lmp;
            }
            if (tid == 0) { sp.frames[b] = t0 + n; sp.nh[b] = nh; }
            if constexpr (TM)
                if (tid == 0 && n > 0) tp.count[b] = a0 + n;     // (every thread read a0 before the first frame's barriers)
            if (tid < N) {
                const int64_t r = (int64_t)b * N + tid;
                int64_t* out = tokens + r * TO;
                int len = 0;
                if (tid < nh) {
                    len = min(h_len[cur][tid], TO);
                    int x = h_node[cur][tid];
                    for (int p = len - 1; p >= 0 && x > 0; --p) {
                        const int2 e = nd[x];
                        out[p] = e.y;
                        if constexpr (TM) {
                            const int2 w = tr[x];
                            tp.token_frames[r * TO + p] = w.x;
                            tp.token_logp[r * TO + p] = __int_as_float(w.y);
                        }
                        x = e.x;
                    }
                }
                scores[r] = (float)f;
                if (sp.am_out) sp.am_out[r] = tid < nh ? (float)h_s[cur][tid] : -INFINITY;
                counts[r] = len;
                for (int p = len; p < TO; ++p) out[p] = -1;
                if constexpr (TM)
                    for (int p = len; p < TO; ++p) { tp.token_frames[r * TO + p] = -1; tp.token_logp[r * TO + p] = -INFINITY; }
            }
            if (tid == 0) num_hyps[b] = min(nh, N);
            return;
        }
    }
    if constexpr (LM || HW) {
        // ---- end of utterance: drop P (and Q), score the partial word and </s>, count the matches with the partial word as
        // the last word; re-rank by the final F (ties to the earlier rank)
        if (tid < nh) {
            double lmf = 0.0;
            if constexpr (LM) {
                lmf = h_lm[cur][tid];
                const int tn = h_tn[cur][tid], pl = h_pl[cur][tid];
                int ctx[LM_CTX];
                for (int i = 0; i < LM_CTX; ++i) ctx[i] = h_ctx[cur][i][tid];
                if (pl > 0) {
                    const int wd = tn >= 0 ? lmv.node_word[tn] : -1;
                    const int w = wd >= 0 ? wd : lmv.unk;
                    lmf = lmf + (lp.alpha * LN10 * (lm_cond_log10(lmv, ctx, w) + (wd >= 0 ? 0.0 : lp.unk_offset)) + lp.beta);
                    lm_ctx_push(ctx, w);
                }
                if (lp.score_boundary) lmf = lmf + lp.alpha * LN10 * lm_cond_log10(lmv, ctx, lmv.eos);
            }
            if constexpr (HW) {
                const int fhn = h_hn[cur][tid];
                int fc = h_hc[cur][tid];
                if (fhn != 0) {
                    int ids[HW_WIN];
#pragma unroll
                    for (int u = 0; u < HW_WIN; ++u) ids[u] = h_hw[cur][u][tid];
                    int wl = h_hwl[cur][tid], dec = h_hd[cur][tid];
                    fc = hw_push(hwv, ids, wl, dec, fhn > 0 ? hwv.cnode[fhn].x : -1);
                }
                lmf = lmf + hww * (double)fc;
            }
            m_val[tid] = h_s[cur][tid] + lmf;
        }
        __syncthreads();
        int r = tid;                                         // rows [nh, N) are padding
        if (tid < nh) {
            const double f = m_val[tid];
            r = 0;
            for (int j = 0; j < nh; ++j) r += m_val[j] > f || (m_val[j] == f && j < tid);
        }
        if (r < N) {
            const int64_t o = (int64_t)b * N + r;
            int64_t* out = tokens + o * TO;
            int len = 0;
            if (tid < nh) {
                len = min(h_len[cur][tid], TO);
                int x = h_node[cur][tid];
                for (int p = len - 1; p >= 0 && x > 0; --p) {
                    const int2 e = nd[x];
                    out[p] = e.y;
                    if constexpr (TM) {
                        const int2 w = tr[x];
                        tp.token_frames[o * TO + p] = w.x;
                        tp.token_logp[o * TO + p] = __int_as_float(w.y);
                    }
                    x = e.x;
                }
                scores[o] = (float)m_val[tid];
                lp.am_scores[o] = (float)h_s[cur][tid];
            } else {
                scores[o] = -INFINITY;
                lp.am_scores[o] = -INFINITY;
            }
            counts[o] = len;
            for (int p = len; p < TO; ++p) out[p] = -1;
            if constexpr (TM)
                for (int p = len; p < TO; ++p) { tp.token_frames[o * TO + p] = -1; tp.token_logp[o * TO + p] = -INFINITY; }
        }
        if (tid == 0) num_hyps[b] = min(nh, N);
        return;
    }
    // ---- traceback: one thread per returned hypothesis
    if (tid < N) {
        const int64_t o = (int64_t)b * N + tid;
        int64_t* out = tokens + o * TO;
        int len = 0;
        if (tid < nh) {
            len = min(h_len[cur][tid], TO);
            int x = h_node[cur][tid];
            for (int p = len - 1; p >= 0 && x > 0; --p) {
                const int2 e = nd[x];
                out[p] = e.y;
                if constexpr (TM) {
                    const int2 w = tr[x];
                    tp.token_frames[o * TO + p] = w.x;
                    tp.token_logp[o * TO + p] = __int_as_float(w.y);
                }
                x = e.x;
            }
            scores[o] = (float)h_s[cur][tid];
        } else {
            scores[o] = -INFINITY;
        }
        counts[o] = len;
        for (int p = len; p < TO; ++p) out[p] = -1;
        if constexpr (TM)
            for (int p = len; p < TO; ++p) { tp.token_frames[o * TO + p] = -1; tp.token_logp[o * TO + p] = -INFINITY; }
    }
    if (tid == 0) num_hyps[b] = min(nh, N);
}

// utterance b of a stream at the empty prefix, the state the one-shot kernel builds before its first frame
template <bool LM, bool HW>
__device__ __forceinline__ void beam_stream_init_one(const BeamWs& ws, const StreamParams<true>& sp, int b, int W,
                                                     const void* lm_tables, int score_boundary) {
    const int64_t o = (int64_t)b * W;
    sp.frames[b] = 0; sp.nh[b] = 1;
    sp.pb[o] = 0.0; sp.pnb[o] = -INFINITY; sp.s[o] = 0.0; sp.hash[o] = ROOT_HASH;
    sp.node[o] = 0; sp.last[o] = -1; sp.len[o] = 0;
    ws.nodes[(int64_t)b * (1 + (int64_t)sp.t_max * W)] = make_int2(-1, -1);
    if constexpr (LM) {
        sp.lm[o] = 0.0; sp.tn[o] = 0; sp.pl[o] = 0;
        for (int i = 0; i < LM_CTX; ++i) sp.ctx[((int64_t)b * LM_CTX + i) * W] = -1;
        if (score_boundary) sp.ctx[((int64_t)b * LM_CTX + LM_CTX - 1) * W] = lm_view(lm_tables).bos;
    }
    if constexpr (HW) {
        sp.hn[o] = 0; sp.hd[o] = 0; sp.hwl[o] = 0; sp.hc[o] = 0;
        for (int u = 0; u < HW_WIN; ++u) sp.hw[((int64_t)b * HW_WIN + u) * W] = -1;
    }
}

// every utterance of a stream at the empty prefix
template <bool LM, bool HW>
__global__ void beam_stream_init_kernel(BeamWs ws, StreamParams<true> sp, int B, int W, const void* lm_tables, int score_boundary) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    beam_stream_init_one<LM, HW>(ws, sp, b, W, lm_tables, score_boundary);
}

// the utterances slots[0 .. n) at the empty prefix (independent streams: a slot reopened); entries outside [0, B) are skipped
template <bool LM, bool HW>
__global__ void beam_stream_reset_slots_kernel(BeamWs ws, StreamParams<true> sp, int B, int W, const void* lm_tables,
                                               int score_boundary, const int64_t* slots, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t b = slots[i];
    if (b < 0 || b >= B) return;
    beam_stream_init_one<LM, HW>(ws, sp, (int)b, W, lm_tables, score_boundary);
}

// Committed-prefix streaming (INTEGRATION.md "Committed-prefix streaming (max_pending)"): the step after a resumable step.  One
// workgroup per utterance on the SAVED state, thread r owns saved hypothesis r.  The search kernel numbers new nodes by
// sp.frames and bounds its walks by the saved lengths, and it compares sequences token by token (same_sequence, the
// traceback), never by node identity: so this kernel may cut the shared prefix off every chain, give each survivor a private
// chain at the bottom of the tree and leave lengths, nodes and the frame count relative to the committed prefix.
//   1. thread 0 walks y_0's chain once into y0 (token, node) per position -- global scratch, not LDS: |y_0| is bounded by
//      max_pending + max_chunk_frames, which no LDS array is
//   2. every thread walks its own chain against y0 for the length of its common prefix with y_0 (it stops where both chains
//      reach the same node: the rest is shared); block-min -> lcp; nb; survivors; their ranks by a ballot scan in rank order
//   3. each survivor copies its pending suffix (<= max_pending tokens) to its own scratch row and reads its saved values
//   4. after the barrier (no thread reads the old tree or the old values any more): the private chains, the values at the
//      survivors' ranks, nh, frames, the commit log and its total
struct CommitParams {
    int2* y0;                            // (B, T_tree) scratch
    int* suf;                            // (B, W, M) scratch
    int* log;                            // (B, L) ring of committed tokens
    int64_t* total;                      // (B) tokens committed so far
    int* committed;                      // (B) tokens committed by this call, or null
    const int64_t* lengths;              // the step's lengths, or null
    int M, L;
};

// TM: the nodes' records (TimesParams::rec) go where their tokens go: y_0's into y0r beside y0, a survivor's pending suffix
// into sufr beside suf and from there into its private chain, and y_0[:nb]'s into the rings log_frames / log_logp at the
// positions of `log`.  The absolute frame count is not touched: a commit consumes no frame.
template <bool TM> struct CommitTimes {};
template <> struct CommitTimes<true> {
    int2* rec;                           // (B, 1 + T_tree*W)
    int2* y0r;                           // (B, T_tree) scratch
    int2* sufr;                          // (B, W, M) scratch
    int64_t* log_frames;                 // (B, L)
    float* log_logp;                     // (B, L)
};

template <bool TM>
__global__ __launch_bounds__(BEAM_MAX_W) void beam_commit_kernel(BeamWs ws, StreamParams<true> sp, CommitParams cp, int W,
                                                                 CommitTimes<TM> ct = {}) {
    __shared__ int red_min[4], red_cnt[4], red_max[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int TT = sp.t_max, M = cp.M;
    const int nh = min(sp.nh[b], W);
    if ((cp.lengths && cp.lengths[b] <= 0) || nh < 1) {                  // no frame consumed: nothing changed (block-uniform)
        if (tid == 0 && cp.committed) cp.committed[b] = 0;
        return;
    }
    const int nn = 1 + TT * W;                                            // nodes of one utterance's tree
    int2* nd = ws.nodes + (int64_t)b * nn;
    int2* y0 = cp.y0 + (int64_t)b * TT;
    const int64_t o = (int64_t)b * W + tid;
    const int64_t tot = cp.total[b];
    const int len0 = min(max(sp.len[(int64_t)b * W], 0), TT);
    [[maybe_unused]] int2 *tr = nullptr, *y0r = nullptr, *sufr = nullptr;
    if constexpr (TM) {
        tr = ct.rec + (int64_t)b * nn;
        y0r = ct.y0r + (int64_t)b * TT;
        sufr = ct.sufr + o * M;
    }
    // ---- 1: y_0's pending tokens and their nodes
    if (tid == 0) {
        int x = sp.node[(int64_t)b * W];
        for (int p = len0 - 1; p >= 0 && x > 0 && x < nn; --p) {
            const int2 e = nd[x];
            y0[p] = make_int2(e.y, x);
            if constexpr (TM) y0r[p] = tr[x];
            x = e.x;
        }
    }
    __syncthreads();
    // ---- 2: common prefix with y_0
    const bool own = tid < nh;
    int len = 0, node = 0, lc = INT_MAX;
    if (own) {
        len = min(max(sp.len[o], 0), TT);
        node = sp.node[o];
        lc = min(len, len0);
        int x = node;
        for (int p = len - 1; p >= 0 && x > 0 && x < nn; --p) {
            const int2 e = nd[x];
            if (p < len0) {
                const int2 y = y0[p];
                if (y.y == x) break;                                      // the same node: both chains are one from here down
                if (y.x != e.y) lc = p;
            }
            x = e.x;
        }
    }
    int m = lc;
#pragma unroll
    for (int q = 32; q > 0; q >>= 1) m = min(m, __shfl_xor(m, q, 64));
    if (lane == 0) red_min[wv] = m;
    __syncthreads();
    const int lcp = min(min(red_min[0], red_min[1]), min(red_min[2], red_min[3]));
    const int nb = max(lcp, len0 - M);                                    // 0 <= nb <= len0 (thread 0 holds lc = len0)
    const bool surv = own && lc >= nb && len - nb <= M;                   // (lc >= nb: y_r starts with y_0[:nb])
    const int slen = surv ? len - nb : 0;
    const unsigned long long bal = __ballot(surv);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    int mx = slen;
#pragma unroll
    for (int q = 32; q > 0; q >>= 1) mx = max(mx, __shfl_xor(mx, q, 64));
    if (lane == 0) { red_cnt[wv] = __popcll(bal); red_max[wv] = mx; }
    // ---- 3: the survivor's suffix to its scratch row, its saved values to registers
    int* suf = cp.suf + o * M;
    double pb = 0, pnb = 0, s = 0, lm = 0;
    unsigned long long hash = 0;
    int last = 0, tn = 0, pl = 0, hn = 0, hd = 0, hwl = 0, hc = 0;
    int ctx[LM_CTX];
    short hw[HW_WIN];
    if (surv) {
        int x = node;
        for (int p = slen - 1; p >= 0 && x > 0 && x < nn; --p) {
            const int2 e = nd[x];
            suf[p] = e.y;
            if constexpr (TM) sufr[p] = tr[x];
            x = e.x;
        }
        pb = sp.pb[o]; pnb = sp.pnb[o]; s = sp.s[o]; hash = sp.hash[o]; last = sp.last[o];
        if (sp.lm) {
            lm = sp.lm[o]; tn = sp.tn[o]; pl = sp.pl[o];
            for (int i = 0; i < LM_CTX; ++i) ctx[i] = sp.ctx[((int64_t)b * LM_CTX + i) * W + tid];
        }
        if (sp.hn) {
            hn = sp.hn[o]; hd = sp.hd[o]; hwl = sp.hwl[o]; hc = sp.hc[o];
            for (int u = 0; u < HW_WIN; ++u) hw[u] = sp.hw[((int64_t)b * HW_WIN + u) * W + tid];
        }
    }
    __syncthreads();
    // ---- 4: private chains and the compacted state
    int q = pre;
    for (int w = 0; w < wv; ++w) q += red_cnt[w];
    if (surv) {
        for (int p = 0; p < slen; ++p) nd[1 + p * W + q] = make_int2(p ? 1 + (p - 1) * W + q : 0, suf[p]);
        if constexpr (TM)
            for (int p = 0; p < slen; ++p) tr[1 + p * W + q] = sufr[p];
        const int64_t oq = (int64_t)b * W + q;
        sp.pb[oq] = pb; sp.pnb[oq] = pnb; sp.s[oq] = s; sp.hash[oq] = hash; sp.last[oq] = last;
        sp.node[oq] = slen ? 1 + (slen - 1) * W + q : 0;
        sp.len[oq] = slen;
        if (sp.lm) {
            sp.lm[oq] = lm; sp.tn[oq] = tn; sp.pl[oq] = pl;
            for (int i = 0; i < LM_CTX; ++i) sp.ctx[((int64_t)b * LM_CTX + i) * W + q] = ctx[i];
        }
        if (sp.hn) {
            sp.hn[oq] = hn; sp.hd[oq] = hd; sp.hwl[oq] = hwl; sp.hc[oq] = hc;
            for (int u = 0; u < HW_WIN; ++u) sp.hw[((int64_t)b * HW_WIN + u) * W + q] = hw[u];
        }
    }
    for (int p = tid; p < nb; p += BEAM_MAX_W) cp.log[(int64_t)b * cp.L + (int)(((tot + p) % cp.L + cp.L) % cp.L)] = y0[p].x;
    if constexpr (TM)
        for (int p = tid; p < nb; p += BEAM_MAX_W) {
            const int64_t at = (int64_t)b * cp.L + (int)(((tot + p) % cp.L + cp.L) % cp.L);
            ct.log_frames[at] = y0r[p].x;
            ct.log_logp[at] = __int_as_float(y0r[p].y);
        }
    if (tid == 0) {
        sp.nh[b] = red_cnt[0] + red_cnt[1] + red_cnt[2] + red_cnt[3];
        sp.frames[b] = max(max(red_max[0], red_max[1]), max(red_max[2], red_max[3]));
        cp.total[b] = tot + nb;
        if (cp.committed) cp.committed[b] = nb;
    }
}

__global__ void beam_commit_reset_slots_kernel(int64_t* total, int B, const int64_t* slots, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t b = slots[i];
    if (b >= 0 && b < B) total[b] = 0;
}

// the commit buffer: the stream state for T_tree = M + k_cap frames, then the commit step's scratch
inline size_t commit_carve(int B, int M, int k_cap, int W, int K, bool lm, bool hw, char* base, BeamWs* ws, StreamParams<true>* sp,
                           CommitParams* cp) {
    const int TT = M + k_cap;
    size_t off = stream_carve(B, TT, W, K, lm, hw, base, ws, sp);
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += beam_align(bytes); return p; };
    char* y0 = take((size_t)B * TT * sizeof(int2));
    char* suf = take((size_t)B * W * M * sizeof(int));
    if (cp) { cp->y0 = (int2*)y0; cp->suf = (int*)suf; cp->M = M; }
    return off;
}

// the frame counts of every utterance (slots null) or of the utterances slots[0 .. n) back at 0; entries outside [0, B) are skipped
__global__ void beam_times_reset_kernel(int64_t* count, int B, const int64_t* slots, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t b = slots ? slots[i] : i;
    if (b >= 0 && b < B) count[b] = 0;
}

// the times buffer: the frame counts and the node records of a tree of T frames, then (M > 0: commit mode) the commit step's
// record scratch.  The search entries need the first two only, so a buffer sized with M serves them too.
struct TimesBuf {
    int64_t* count;
    int2 *rec, *y0r, *sufr;
};

inline size_t times_carve(int B, int T, int W, int M, char* base, TimesBuf* tb) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += beam_align(bytes); return p; };
    char* count = take((size_t)B * sizeof(int64_t));
    char* rec = take((size_t)B * (1 + (size_t)T * W) * sizeof(int2));
    char *y0r = nullptr, *sufr = nullptr;
    if (M > 0) {
        y0r = take((size_t)B * T * sizeof(int2));
        sufr = take((size_t)B * W * M * sizeof(int2));
    }
    if (tb) *tb = TimesBuf{(int64_t*)count, (int2*)rec, (int2*)y0r, (int2*)sufr};
    return off;
}

inline bool times_args_ok(int B, int T, int W, int M) {
    return B > 0 && T > 0 && W >= 1 && W <= BEAM_MAX_W && (int64_t)T * W < INT32_MAX && M >= 0 && (M == 0 || M < T);
}

inline bool commit_args_ok(int B, int M, int k_cap, int W, int K) {
    return B > 0 && M >= 1 && k_cap >= 1 && W >= 1 && W <= BEAM_MAX_W && K >= 1 && K <= BEAM_MAX_K &&
           ((int64_t)M + k_cap) * W < INT32_MAX;
}

// ---- host side ---------------------------------------------------------------------------------------------------------

#define CFM_CHECK(call) do { const int st_ = (call); if (st_ != CFM_OK) return st_; } while (0)

// The argument rules every search entry shares, in the order their statuses are reported.  T: the frames the tree has room
// for (T_max for the stream entries).  The entries without logits pass V = 2, blank = 0 and zero knobs, which always pass;
// the stream init (no outputs) also passes N = 1.
int beam_check(int B, int T, int V, int W, int K, int N, int blank, float token_min_logp, float beam_prune_logp) {
    CFM_REQUIRE(B > 0 && T > 0 && V >= 2, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(W >= 1 && W <= BEAM_MAX_W, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE(K >= 1 && K <= BEAM_MAX_K, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE(N >= 1 && N <= W, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(blank >= 0 && blank < V, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(V <= BEAM_MAX_V && (int64_t)T * W < INT32_MAX, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE(!(token_min_logp != token_min_logp) && !(beam_prune_logp != beam_prune_logp), CFM_ERR_BAD_SHAPE);   // NaN
    return CFM_OK;
}

// the fusion arguments of the C entries; a null table pointer leaves that term out (the LM-only entry passes weight 0)
struct Fusion {
    const void* lm_tables;
    double alpha, beta, unk;
    int score_boundary;
    const void* hw_tables;
    double hw_weight;
    const void* const* hw_rows = nullptr;            // per-request hotwords: hw_tables is then the mode flag only
    const double* hw_row_weights = nullptr;
    bool on() const { return lm_tables || hw_tables; }
    bool finite() const {
        return __builtin_isfinite(alpha) && __builtin_isfinite(beta) && __builtin_isfinite(unk) && __builtin_isfinite(hw_weight);
    }
};

// f(std::bool_constant<LM>{}, std::bool_constant<HW>{}) in the mode the table pointers select
template <class F> void beam_mode(const Fusion& fz, F&& f) {
    if (fz.lm_tables && fz.hw_tables) f(std::true_type{}, std::true_type{});
    else if (fz.lm_tables) f(std::true_type{}, std::false_type{});
    else if (fz.hw_tables) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
}

// the fusion group as the search of mode <LM, HW> takes it (tables is null in the hotword-only form)
template <bool LM, bool HW> LmParams<LM, HW> lm_params(const Fusion& fz, float* am_scores) {
    LmParams<LM, HW> lp{};
    if constexpr (LM || HW) {
        lp.tables = fz.lm_tables;
        lp.alpha = fz.alpha; lp.beta = fz.beta; lp.unk_offset = fz.unk;
        lp.score_boundary = fz.score_boundary ? 1 : 0;
        lp.am_scores = am_scores;
    }
    if constexpr (HW) {
        lp.hw_tables = fz.hw_tables; lp.hw_weight = fz.hw_weight;
        lp.hw_rows = fz.hw_rows; lp.hw_row_weights = fz.hw_row_weights;
    }
    return lp;
}

// The candidate rows of the T frames (none for T = 0: the finish), then the search in the mode fz selects; ST: the resumable
// search on the stream state sp.
template <bool ST, bool TM = false>
int beam_launch(const float* logits, const int64_t* lengths, const BeamWs& ws, StreamParams<ST> sp, int B, int T, int V,
                int blank, int W, int K, float token_min_logp, float beam_prune_logp, int N, const Fusion& fz, int64_t* tokens,
                int64_t* counts, float* scores, float* am_scores, int64_t* num_hyps, cfm_stream_t stream,
                TimesParams<TM> tp = {}) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (T > 0) {
        const int64_t rows = (int64_t)B * T;
        hipLaunchKernelGGL(beam_prep_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits, lengths, ws, B, T, V,
                           blank, K, (double)token_min_logp);
    }
    beam_mode(fz, [&](auto lm, auto hw) {
        constexpr bool LM = decltype(lm)::value, HW = decltype(hw)::value;
        hipLaunchKernelGGL((beam_search_kernel<LM, HW, ST, TM>), dim3((unsigned)B), dim3(BEAM_MAX_W), 0, s, logits, lengths, ws,
                           T, V, blank, W, K, (double)beam_prune_logp, N, tokens, counts, scores, num_hyps,
                           lm_params<LM, HW>(fz, am_scores), sp, tp);
    });
    return cfm_launch_status();
}

// the one-shot search of cfm_ctc_beam_{,lm_,hw_}decode_f32 after their pointer checks
int beam_decode(const float* logits, const int64_t* lengths, int B, int T, int V, int blank, int W, int K, float token_min_logp,
                float beam_prune_logp, int N, const Fusion& fz, void* workspace, size_t workspace_bytes, int64_t* tokens,
                int64_t* counts, float* scores, float* am_scores, int64_t* num_hyps, cfm_stream_t stream) {
    CFM_CHECK(beam_check(B, T, V, W, K, N, blank, token_min_logp, beam_prune_logp));
    CFM_REQUIRE(!fz.on() || fz.finite(), CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(workspace_bytes >= beam_carve(B, T, W, K, nullptr, nullptr), CFM_ERR_BAD_SHAPE);
    BeamWs ws;
    beam_carve(B, T, W, K, static_cast<char*>(workspace), &ws);
    return beam_launch(logits, lengths, ws, StreamParams<false>{}, B, T, V, blank, W, K, token_min_logp, beam_prune_logp, N, fz,
                       tokens, counts, scores, am_scores, num_hyps, stream);
}

// the stream buffer of the mode fz selects, carved (BAD_SHAPE when it is too small)
int stream_state(int B, int T_max, int W, int K, const Fusion& fz, void* state, size_t state_bytes, BeamWs* ws,
                 StreamParams<true>* sp) {
    const bool lm = fz.lm_tables != nullptr, hw = fz.hw_tables != nullptr;
    CFM_REQUIRE(state_bytes >= stream_carve(B, T_max, W, K, lm, hw, nullptr, nullptr, nullptr), CFM_ERR_BAD_SHAPE);
    stream_carve(B, T_max, W, K, lm, hw, static_cast<char*>(state), ws, sp);
    return CFM_OK;
}

}  // namespace

extern "C" size_t cfm_ctc_beam_workspace_bytes(int B, int T, int W, int K) {
    if (B <= 0 || T <= 0 || W < 1 || W > BEAM_MAX_W || K < 1 || K > BEAM_MAX_K) return 0;
    return beam_carve(B, T, W, K, nullptr, nullptr);
}

extern "C" int cfm_ctc_beam_decode_f32(const float* logits, const int64_t* lengths_or_null, int B, int T, int V, int blank_id,
                                       int beam_width, int max_candidates, float token_min_logp, float beam_prune_logp,
                                       int n_best, void* workspace, size_t workspace_bytes, int64_t* tokens, int64_t* counts,
                                       float* scores, int64_t* num_hyps, cfm_stream_t stream) {
    CFM_REQUIRE(logits && workspace && tokens && counts && scores && num_hyps, CFM_ERR_NULL);
    return beam_decode(logits, lengths_or_null, B, T, V, blank_id, beam_width, max_candidates, token_min_logp, beam_prune_logp,
                       n_best, Fusion{}, workspace, workspace_bytes, tokens, counts, scores, nullptr, num_hyps, stream);
}

extern "C" size_t cfm_ctc_beam_lm_workspace_bytes(int B, int T, int W, int K) {
    return cfm_ctc_beam_workspace_bytes(B, T, W, K);
}

extern "C" int cfm_ctc_beam_lm_decode_f32(const float* logits, const int64_t* lengths_or_null, int B, int T, int V, int blank_id,
                                          int beam_width, int max_candidates, float token_min_logp, float beam_prune_logp,
                                          int n_best, const void* lm_tables, double alpha, double beta, double unk_score_offset,
                                          int score_boundary, void* workspace, size_t workspace_bytes, int64_t* tokens,
                                          int64_t* counts, float* scores, float* am_scores, int64_t* num_hyps,
                                          cfm_stream_t stream) {
    CFM_REQUIRE(logits && lm_tables && workspace && tokens && counts && scores && am_scores && num_hyps, CFM_ERR_NULL);
    return beam_decode(logits, lengths_or_null, B, T, V, blank_id, beam_width, max_candidates, token_min_logp, beam_prune_logp,
                       n_best, Fusion{lm_tables, alpha, beta, unk_score_offset, score_boundary, nullptr, 0.0}, workspace,
                       workspace_bytes, tokens, counts, scores, am_scores, num_hyps, stream);
}

extern "C" size_t cfm_ctc_beam_hw_workspace_bytes(int B, int T, int W, int K) {
    return cfm_ctc_beam_workspace_bytes(B, T, W, K);
}

extern "C" int cfm_ctc_beam_hw_decode_f32(const float* logits, const int64_t* lengths_or_null, int B, int T, int V, int blank_id,
                                          int beam_width, int max_candidates, float token_min_logp, float beam_prune_logp,
                                          int n_best, const void* lm_tables_or_null, double alpha, double beta,
                                          double unk_score_offset, int score_boundary, const void* hw_tables,
                                          double hotword_weight, void* workspace, size_t workspace_bytes, int64_t* tokens,
                                          int64_t* counts, float* scores, float* am_scores, int64_t* num_hyps,
                                          cfm_stream_t stream) {
    CFM_REQUIRE(logits && hw_tables && workspace && tokens && counts && scores && am_scores && num_hyps, CFM_ERR_NULL);
    const Fusion fz{lm_tables_or_null, alpha, beta, unk_score_offset, score_boundary, hw_tables, hotword_weight};
    return beam_decode(logits, lengths_or_null, B, T, V, blank_id, beam_width, max_candidates, token_min_logp, beam_prune_logp,
                       n_best, fz, workspace, workspace_bytes, tokens, counts, scores, am_scores, num_hyps, stream);
}

// ---- streaming (resumable) search ----------------------------------------------------------------------------------------

extern "C" size_t cfm_ctc_beam_stream_state_bytes(int B, int T_max, int W, int K, int lm, int hw) {
    if (B <= 0 || T_max <= 0 || W < 1 || W > BEAM_MAX_W || K < 1 || K > BEAM_MAX_K || (int64_t)T_max * W >= INT32_MAX) return 0;
    return stream_carve(B, T_max, W, K, lm != 0, hw != 0, nullptr, nullptr, nullptr);
}

extern "C" int cfm_ctc_beam_stream_init(int B, int T_max, int beam_width, int max_candidates, const void* lm_tables_or_null,
                                        int score_boundary, const void* hw_tables_or_null, void* state, size_t state_bytes,
                                        cfm_stream_t stream) {
    CFM_REQUIRE(state, CFM_ERR_NULL);
    CFM_CHECK(beam_check(B, T_max, 2, beam_width, max_candidates, 1, 0, 0.f, 0.f));
    const Fusion fz{lm_tables_or_null, 0.0, 0.0, 0.0, score_boundary, hw_tables_or_null, 0.0};
    BeamWs ws;
    StreamParams<true> sp;
    CFM_CHECK(stream_state(B, T_max, beam_width, max_candidates, fz, state, state_bytes, &ws, &sp));
    const int sb = score_boundary ? 1 : 0;
    beam_mode(fz, [&](auto lm, auto hw) {
        hipLaunchKernelGGL((beam_stream_init_kernel<decltype(lm)::value, decltype(hw)::value>), dim3((unsigned)((B + 255) / 256)),
                           dim3(256), 0, static_cast<hipStream_t>(stream), ws, sp, B, beam_width, lm_tables_or_null, sb);
    });
    return cfm_launch_status();
}

// independent streams (conformer_amd/slots.py): the utterances slots[0 .. n_slots) back at the empty prefix, the others untouched.
// The step's `t_used` is a bound only; with slots at different positions the caller passes max_b(frames_b + lengths_b) - Tc.
extern "C" int cfm_ctc_beam_stream_reset_slots(int B, int T_max, int beam_width, int max_candidates, const void* lm_tables_or_null,
                                               int score_boundary, const void* hw_tables_or_null, const int64_t* slots,
                                               int n_slots, void* state, size_t state_bytes, cfm_stream_t stream) {
    CFM_REQUIRE(state && slots, CFM_ERR_NULL);
    CFM_CHECK(beam_check(B, T_max, 2, beam_width, max_candidates, 1, 0, 0.f, 0.f));
    CFM_REQUIRE(n_slots >= 1 && n_slots <= B, CFM_ERR_BAD_SHAPE);
    const Fusion fz{lm_tables_or_null, 0.0, 0.0, 0.0, score_boundary, hw_tables_or_null, 0.0};
    BeamWs ws;
    StreamParams<true> sp;
    CFM_CHECK(stream_state(B, T_max, beam_width, max_candidates, fz, state, state_bytes, &ws, &sp));
    const int sb = score_boundary ? 1 : 0;
    beam_mode(fz, [&](auto lm, auto hw) {
        hipLaunchKernelGGL((beam_stream_reset_slots_kernel<decltype(lm)::value, decltype(hw)::value>),
                           dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), ws, sp, B,
                           beam_width, lm_tables_or_null, sb, slots, n_slots);
    });
    return cfm_launch_status();
}

namespace {

// the times arguments of the *_times entries (include/conformer_hip_times.h); a null TimesArgs is the entry without them
struct TimesArgs {
    void* times;
    size_t bytes;
    int64_t* token_frames;
    float* token_logp;
    bool null() const { return !times || !token_frames || !token_logp; }
};

// the search's view of a times buffer over a tree of T frames (BAD_SHAPE when it is too small)
int times_params(const TimesArgs& ta, int B, int T, int W, TimesParams<true>* tp) {
    CFM_REQUIRE(times_args_ok(B, T, W, 0) && ta.bytes >= times_carve(B, T, W, 0, nullptr, nullptr), CFM_ERR_BAD_SHAPE);
    TimesBuf tb;
    times_carve(B, T, W, 0, static_cast<char*>(ta.times), &tb);
    *tp = TimesParams<true>{tb.count, tb.rec, ta.token_frames, ta.token_logp};
    return CFM_OK;
}

int stream_step(const float* logits, const int64_t* lengths_or_null, int B, int Tc, int V, int blank_id, int beam_width,
                int max_candidates, float token_min_logp, float beam_prune_logp, int n_best, const Fusion& fz, void* state,
                size_t state_bytes, int T_max, int t_used, int64_t* tokens, int64_t* counts, float* scores,
                float* am_scores_or_null, int64_t* num_hyps, cfm_stream_t stream, const TimesArgs* ta) {
    CFM_REQUIRE(logits && state && tokens && counts && scores && num_hyps && !(ta && ta->null()), CFM_ERR_NULL);
    CFM_REQUIRE(Tc > 0, CFM_ERR_BAD_SHAPE);
    CFM_CHECK(beam_check(B, T_max, V, beam_width, max_candidates, n_best, blank_id, token_min_logp, beam_prune_logp));
    // t_used: chunk frames passed to the earlier steps since the init, a bound on what any utterance consumed
    CFM_REQUIRE(t_used >= 0 && t_used <= T_max && Tc <= T_max - t_used, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(fz.finite(), CFM_ERR_BAD_SHAPE);
    BeamWs ws;
    StreamParams<true> sp;
    CFM_CHECK(stream_state(B, T_max, beam_width, max_candidates, fz, state, state_bytes, &ws, &sp));
    sp.am_out = am_scores_or_null;
    sp.finish = 0;
    if (ta) {
        TimesParams<true> tp;
        CFM_CHECK(times_params(*ta, B, T_max, beam_width, &tp));
        return beam_launch<true, true>(logits, lengths_or_null, ws, sp, B, Tc, V, blank_id, beam_width, max_candidates,
                                       token_min_logp, beam_prune_logp, n_best, fz, tokens, counts, scores, am_scores_or_null,
                                       num_hyps, stream, tp);
    }
    return beam_launch(logits, lengths_or_null, ws, sp, B, Tc, V, blank_id, beam_width, max_candidates, token_min_logp,
                       beam_prune_logp, n_best, fz, tokens, counts, scores, am_scores_or_null, num_hyps, stream);
}

int stream_finish(int B, int beam_width, int max_candidates, int n_best, const Fusion& fz, void* state, size_t state_bytes,
                  int T_max, int64_t* tokens, int64_t* counts, float* scores, float* am_scores_or_null, int64_t* num_hyps,
                  cfm_stream_t stream, const TimesArgs* ta) {
    CFM_REQUIRE(state && tokens && counts && scores && num_hyps && (am_scores_or_null || !fz.on()) && !(ta && ta->null()),
                CFM_ERR_NULL);
    CFM_CHECK(beam_check(B, T_max, 2, beam_width, max_candidates, n_best, 0, 0.f, 0.f));
    CFM_REQUIRE(fz.finite(), CFM_ERR_BAD_SHAPE);
    BeamWs ws;
    StreamParams<true> sp;
    CFM_CHECK(stream_state(B, T_max, beam_width, max_candidates, fz, state, state_bytes, &ws, &sp));
    sp.am_out = nullptr;
    sp.finish = 1;
    // no frames: the kernel resumes the saved state and goes straight to the end-of-utterance step (LM / hotwords) or the
    // traceback (plain search)
    if (ta) {
        TimesParams<true> tp;
        CFM_CHECK(times_params(*ta, B, T_max, beam_width, &tp));
        return beam_launch<true, true>(nullptr, nullptr, ws, sp, B, 0, 2, 0, beam_width, max_candidates, 0.f, 0.f, n_best, fz,
                                       tokens, counts, scores, am_scores_or_null, num_hyps, stream, tp);
    }
    return beam_launch(nullptr, nullptr, ws, sp, B, 0, 2, 0, beam_width, max_candidates, 0.f, 0.f, n_best, fz, tokens, counts,
                       scores, am_scores_or_null, num_hyps, stream);
}

}  // namespace

extern "C" int cfm_ctc_beam_stream_step_f32(const float* logits, const int64_t* lengths_or_null, int B, int Tc, int V,
                                            int blank_id, int beam_width, int max_candidates, float token_min_logp,
                                            float beam_prune_logp, int n_best, const void* lm_tables_or_null, double alpha,
                                            double beta, double unk_score_offset, int score_boundary,
                                            const void* hw_tables_or_null, double hotword_weight, void* state,
                                            size_t state_bytes, int T_max, int t_used, int64_t* tokens, int64_t* counts,
                                            float* scores, float* am_scores_or_null, int64_t* num_hyps, cfm_stream_t stream) {
    const Fusion fz{lm_tables_or_null, alpha, beta, unk_score_offset, score_boundary, hw_tables_or_null, hotword_weight};
    return stream_step(logits, lengths_or_null, B, Tc, V, blank_id, beam_width, max_candidates, token_min_logp, beam_prune_logp,
                       n_best, fz, state, state_bytes, T_max, t_used, tokens, counts, scores, am_scores_or_null, num_hyps, stream,
                       nullptr);
}

extern "C" int cfm_ctc_beam_stream_finish_f32(int B, int beam_width, int max_candidates, int n_best, const void* lm_tables_or_null,
                                              double alpha, double beta, double unk_score_offset, int score_boundary,
                                              const void* hw_tables_or_null, double hotword_weight, void* state,
                                              size_t state_bytes, int T_max, int64_t* tokens, int64_t* counts, float* scores,
                                              float* am_scores_or_null, int64_t* num_hyps, cfm_stream_t stream) {
    const Fusion fz{lm_tables_or_null, alpha, beta, unk_score_offset, score_boundary, hw_tables_or_null, hotword_weight};
    return stream_finish(B, beam_width, max_candidates, n_best, fz, state, state_bytes, T_max, tokens, counts, scores,
                         am_scores_or_null, num_hyps, stream, nullptr);
}

// ---- committed-prefix streaming (include/conformer_hip_commit.h) ----------------------------------------------------------------

extern "C" size_t cfm_ctc_beam_commit_state_bytes(int B, int max_pending, int max_chunk_frames, int W, int K, int lm, int hw) {
    if (!commit_args_ok(B, max_pending, max_chunk_frames, W, K)) return 0;
    return commit_carve(B, max_pending, max_chunk_frames, W, K, lm != 0, hw != 0, nullptr, nullptr, nullptr, nullptr);
}

namespace {

// ta: the times buffer and, in its output fields, the rings log_frames / log_logp (null: the commit without them)
int stream_commit(int B, int max_pending, int max_chunk_frames, int beam_width, int max_candidates, int lm, int hw,
                  const int64_t* lengths_or_null, void* state, size_t state_bytes, int* log, int L, int64_t* total,
                  int* committed_or_null, cfm_stream_t stream, const TimesArgs* ta) {
    CFM_REQUIRE(state && log && total && !(ta && ta->null()), CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && max_pending >= 1 && max_chunk_frames >= 1, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE((int64_t)max_pending + max_chunk_frames < INT32_MAX, CFM_ERR_UNSUPPORTED);
    const int TT = max_pending + max_chunk_frames;
    CFM_CHECK(beam_check(B, TT, 2, beam_width, max_candidates, 1, 0, 0.f, 0.f));
    CFM_REQUIRE(L >= TT, CFM_ERR_BAD_SHAPE);
    BeamWs ws;
    StreamParams<true> sp;
    CommitParams cp{};
    CFM_REQUIRE(state_bytes >= commit_carve(B, max_pending, max_chunk_frames, beam_width, max_candidates, lm != 0, hw != 0, nullptr,
                                            nullptr, nullptr, nullptr), CFM_ERR_BAD_SHAPE);
    commit_carve(B, max_pending, max_chunk_frames, beam_width, max_candidates, lm != 0, hw != 0, static_cast<char*>(state), &ws,
                 &sp, &cp);
    cp.log = log; cp.L = L; cp.total = total; cp.committed = committed_or_null; cp.lengths = lengths_or_null;
    if (ta) {
        CFM_REQUIRE(times_args_ok(B, TT, beam_width, max_pending) &&
                    ta->bytes >= times_carve(B, TT, beam_width, max_pending, nullptr, nullptr), CFM_ERR_BAD_SHAPE);
        TimesBuf tb;
        times_carve(B, TT, beam_width, max_pending, static_cast<char*>(ta->times), &tb);
        const CommitTimes<true> ct{tb.rec, tb.y0r, tb.sufr, ta->token_frames, ta->token_logp};
        hipLaunchKernelGGL(beam_commit_kernel<true>, dim3((unsigned)B), dim3(BEAM_MAX_W), 0, static_cast<hipStream_t>(stream), ws,
                           sp, cp, beam_width, ct);
        return cfm_launch_status();
    }
    hipLaunchKernelGGL(beam_commit_kernel<false>, dim3((unsigned)B), dim3(BEAM_MAX_W), 0, static_cast<hipStream_t>(stream), ws, sp,
                       cp, beam_width, CommitTimes<false>{});
    return cfm_launch_status();
}

}  // namespace

extern "C" int cfm_ctc_beam_stream_commit(int B, int max_pending, int max_chunk_frames, int beam_width, int max_candidates, int lm,
                                          int hw, const int64_t* lengths_or_null, void* state, size_t state_bytes, int* log, int L,
                                          int64_t* total, int* committed_or_null, cfm_stream_t stream) {
    return stream_commit(B, max_pending, max_chunk_frames, beam_width, max_candidates, lm, hw, lengths_or_null, state, state_bytes,
                         log, L, total, committed_or_null, stream, nullptr);
}

extern "C" int cfm_ctc_beam_commit_reset_slots(int B, const int64_t* slots, int n_slots, int64_t* total, cfm_stream_t stream) {
    CFM_REQUIRE(slots && total, CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && n_slots >= 1 && n_slots <= B, CFM_ERR_BAD_SHAPE);
    hipLaunchKernelGGL(beam_commit_reset_slots_kernel, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), total, B, slots, n_slots);
    return cfm_launch_status();
}

// ---- beam-search timestamps (include/conformer_hip_times.h) ----------------------------------------------------------------------

extern "C" size_t cfm_ctc_beam_times_bytes(int B, int T, int W, int max_pending_or_0) {
    if (!times_args_ok(B, T, W, max_pending_or_0)) return 0;
    return times_carve(B, T, W, max_pending_or_0, nullptr, nullptr);
}

extern "C" int cfm_ctc_beam_times_reset(int B, const int64_t* slots_or_null, int n_slots, void* times, size_t times_bytes,
                                        cfm_stream_t stream) {
    CFM_REQUIRE(times, CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && (slots_or_null ? n_slots >= 1 && n_slots <= B : n_slots == 0), CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(times_bytes >= beam_align((size_t)B * sizeof(int64_t)), CFM_ERR_BAD_SHAPE);
    const int n = slots_or_null ? n_slots : B;
    hipLaunchKernelGGL(beam_times_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<int64_t*>(times), B, slots_or_null, n);
    return cfm_launch_status();
}

extern "C" int cfm_ctc_beam_stream_step_times_f32(const float* logits, const int64_t* lengths_or_null, int B, int Tc, int V,
                                                  int blank_id, int beam_width, int max_candidates, float token_min_logp,
                                                  float beam_prune_logp, int n_best, const void* lm_tables_or_null, double alpha,
                                                  double beta, double unk_score_offset, int score_boundary,
                                                  const void* hw_tables_or_null, double hotword_weight, void* state,
                                                  size_t state_bytes, int T_max, int t_used, int64_t* tokens, int64_t* counts,
                                                  float* scores, float* am_scores_or_null, int64_t* num_hyps, void* times,
                                                  size_t times_bytes, int64_t* token_frames, float* token_logp,
                                                  cfm_stream_t stream) {
    const Fusion fz{lm_tables_or_null, alpha, beta, unk_score_offset, score_boundary, hw_tables_or_null, hotword_weight};
    const TimesArgs ta{times, times_bytes, token_frames, token_logp};
    return stream_step(logits, lengths_or_null, B, Tc, V, blank_id, beam_width, max_candidates, token_min_logp, beam_prune_logp,
                       n_best, fz, state, state_bytes, T_max, t_used, tokens, counts, scores, am_scores_or_null, num_hyps, stream,
                       &ta);
}

extern "C" int cfm_ctc_beam_stream_finish_times_f32(int B, int beam_width, int max_candidates, int n_best,
                                                    const void* lm_tables_or_null, double alpha, double beta,
                                                    double unk_score_offset, int score_boundary, const void* hw_tables_or_null,
                                                    double hotword_weight, void* state, size_t state_bytes, int T_max,
                                                    int64_t* tokens, int64_t* counts, float* scores, float* am_scores_or_null,
                                                    int64_t* num_hyps, void* times, size_t times_bytes, int64_t* token_frames,
                                                    float* token_logp, cfm_stream_t stream) {
    const Fusion fz{lm_tables_or_null, alpha, beta, unk_score_offset, score_boundary, hw_tables_or_null, hotword_weight};
    const TimesArgs ta{times, times_bytes, token_frames, token_logp};
    return stream_finish(B, beam_width, max_candidates, n_best, fz, state, state_bytes, T_max, tokens, counts, scores,
                         am_scores_or_null, num_hyps, stream, &ta);
}

extern "C" int cfm_ctc_beam_stream_commit_times(int B, int max_pending, int max_chunk_frames, int beam_width, int max_candidates,
                                                int lm, int hw, const int64_t* lengths_or_null, void* state, size_t state_bytes,
                                                int* log, int L, int64_t* total, int* committed_or_null, void* times,
                                                size_t times_bytes, int64_t* log_frames, float* log_logp, cfm_stream_t stream) {
    const TimesArgs ta{times, times_bytes, log_frames, log_logp};
    return stream_commit(B, max_pending, max_chunk_frames, beam_width, max_candidates, lm, hw, lengths_or_null, state, state_bytes,
                         log, L, total, committed_or_null, stream, &ta);
}

// ---- per-request hotwords (conformer_hip3_hotword_rows.h) ------------------------------------------------------------------------

namespace {

// the fusion group of the per-row entries: the mode is <LM?, HW>, the launch-wide pair is never read (hw_tables is the flag)
Fusion rows_fusion(const void* lm_tables_or_null, double alpha, double beta, double unk_score_offset, int score_boundary,
                   const void* const* hw_row_tables, const double* hw_row_weights) {
    Fusion fz{lm_tables_or_null, alpha, beta, unk_score_offset, score_boundary, hw_row_tables, 0.0};
    fz.hw_rows = hw_row_tables;
    fz.hw_row_weights = hw_row_weights;
    return fz;
}

// the nullable times group of the per-row stream entries: whole (1), absent (0) or neither (-1)
int times_group(const void* times, size_t times_bytes, const int64_t* token_frames, const float* token_logp) {
    if (times && token_frames && token_logp) return 1;
    return !times && !times_bytes && !token_frames && !token_logp ? 0 : -1;
}

}  // namespace

extern "C" int cfm3_ctc_beam_hw_rows_decode_f32(const float* logits, const int64_t* lengths_or_null, int B, int T, int V,
                                                int blank_id, int beam_width, int max_candidates, float token_min_logp,
                                                float beam_prune_logp, int n_best, const void* lm_tables_or_null, double alpha,
                                                double beta, double unk_score_offset, int score_boundary,
                                                const void* const* hw_row_tables, const double* hw_row_weights, void* workspace,
                                                size_t workspace_bytes, int64_t* tokens, int64_t* counts, float* scores,
                                                float* am_scores, int64_t* num_hyps, cfm_stream_t stream) {
    CFM_REQUIRE(logits && hw_row_tables && hw_row_weights && workspace && tokens && counts && scores && am_scores && num_hyps,
                CFM_ERR_NULL);
    const Fusion fz = rows_fusion(lm_tables_or_null, alpha, beta, unk_score_offset, score_boundary, hw_row_tables, hw_row_weights);
    return beam_decode(logits, lengths_or_null, B, T, V, blank_id, beam_width, max_candidates, token_min_logp, beam_prune_logp,
                       n_best, fz, workspace, workspace_bytes, tokens, counts, scores, am_scores, num_hyps, stream);
}

extern "C" int cfm3_ctc_beam_hw_rows_stream_step_f32(const float* logits, const int64_t* lengths_or_null, int B, int Tc, int V,
                                                     int blank_id, int beam_width, int max_candidates, float token_min_logp,
                                                     float beam_prune_logp, int n_best, const void* lm_tables_or_null,
                                                     double alpha, double beta, double unk_score_offset, int score_boundary,
                                                     const void* const* hw_row_tables, const double* hw_row_weights, void* state,
                                                     size_t state_bytes, int T_max, int t_used, int64_t* tokens, int64_t* counts,
                                                     float* scores, float* am_scores_or_null, int64_t* num_hyps,
                                                     void* times_or_null, size_t times_bytes, int64_t* token_frames_or_null,
                                                     float* token_logp_or_null, cfm_stream_t stream) {
    const int tg = times_group(times_or_null, times_bytes, token_frames_or_null, token_logp_or_null);
    CFM_REQUIRE(hw_row_tables && hw_row_weights && tg >= 0, CFM_ERR_NULL);
    const Fusion fz = rows_fusion(lm_tables_or_null, alpha, beta, unk_score_offset, score_boundary, hw_row_tables, hw_row_weights);
    const TimesArgs ta{times_or_null, times_bytes, token_frames_or_null, token_logp_or_null};
    return stream_step(logits, lengths_or_null, B, Tc, V, blank_id, beam_width, max_candidates, token_min_logp, beam_prune_logp,
                       n_best, fz, state, state_bytes, T_max, t_used, tokens, counts, scores, am_scores_or_null, num_hyps, stream,
                       tg ? &ta : nullptr);
}

extern "C" int cfm3_ctc_beam_hw_rows_stream_finish_f32(int B, int beam_width, int max_candidates, int n_best,
                                                       const void* lm_tables_or_null, double alpha, double beta,
                                                       double unk_score_offset, int score_boundary,
                                                       const void* const* hw_row_tables, const double* hw_row_weights,
                                                       void* state, size_t state_bytes, int T_max, int64_t* tokens,
                                                       int64_t* counts, float* scores, float* am_scores, int64_t* num_hyps,
                                                       void* times_or_null, size_t times_bytes, int64_t* token_frames_or_null,
                                                       float* token_logp_or_null, cfm_stream_t stream) {
    const int tg = times_group(times_or_null, times_bytes, token_frames_or_null, token_logp_or_null);
    CFM_REQUIRE(hw_row_tables && hw_row_weights && tg >= 0, CFM_ERR_NULL);
    const Fusion fz = rows_fusion(lm_tables_or_null, alpha, beta, unk_score_offset, score_boundary, hw_row_tables, hw_row_weights);
    const TimesArgs ta{times_or_null, times_bytes, token_frames_or_null, token_logp_or_null};
    return stream_finish(B, beam_width, max_candidates, n_best, fz, state, state_bytes, T_max, tokens, counts, scores, am_scores,
                         num_hyps, stream, tg ? &ta : nullptr);
}
