// Word n-gram language model for CTC beam-search fusion: the host packer of the device tables (layout and hash in
// ngram_lm.h) and a device sentence scorer that reads them.  conformer_amd/lm.py reads ARPA files and calls both; the fused
// search itself is in ctc_beam.hip.
#include <string.h>
#include <vector>
#include "cfm_common.h"
#include "ngram_lm.h"

namespace {

inline int64_t lm_align(int64_t x) { return (x + 255) & ~int64_t(255); }

// slots of an open-addressing table for `count` keys: a power of two >= 2 count (load factor <= 1/2), at least 2
inline int64_t lm_capacity(int64_t count) {
    int64_t cap = 2;
    while (cap < 2 * count) cap <<= 1;
    return cap;
}

constexpr int64_t LM_MAX_SLOTS = int64_t(1) << 31;      // masks are uint32

// byte layout of the blob; 0 if the sizes are out of range
int64_t lm_layout(int order, const int64_t* counts, int n_words, int64_t word_cp_total, int V, int64_t tok_cp_total,
                  LmHeader* h) {
    if (order < 1 || order > LM_MAX_ORDER || !counts || n_words < 1 || word_cp_total < 0 || V < 1 || tok_cp_total < 0)
        return 0;
    if (counts[0] != n_words || word_cp_total >= INT32_MAX || tok_cp_total >= INT32_MAX) return 0;
    LmHeader hd;
    memset(&hd, 0, sizeof(hd));
    int64_t off = lm_align(sizeof(LmHeader));
    for (int n = 0; n < order; ++n) {
        if (counts[n] < 0 || counts[n] > LM_MAX_SLOTS / 2) return 0;
        const int64_t cap = lm_capacity(counts[n]);
        hd.gram_off[n] = off;
        hd.gram_mask[n] = (uint32_t)(cap - 1);
        off = lm_align(off + cap * LM_GRAM_SLOT * 4);
    }
    const int64_t tcap = lm_capacity(word_cp_total);
    hd.trie_off = off;
    hd.trie_mask = (uint32_t)(tcap - 1);
    off = lm_align(off + tcap * 16);
    hd.node_word_off = off;
    off = lm_align(off + (1 + word_cp_total) * 4);
    hd.tok_off_off = off;
    off = lm_align(off + ((int64_t)V + 1) * 4);
    hd.tok_cp_off = off;
    off = lm_align(off + tok_cp_total * 4);
    hd.tok_kind_off = off;
    off = lm_align(off + (int64_t)V * 4);
    hd.magic = LM_MAGIC;
    hd.order = order;
    hd.V = V;
    hd.n_words = n_words;
    hd.total_bytes = off;
    if (h) *h = hd;
    return off;
}

bool offsets_ok(const int64_t* o, int64_t n, int64_t total) {
    if (o[0] != 0 || o[n] != total) return false;
    for (int64_t i = 0; i < n; ++i)
        if (o[i + 1] < o[i]) return false;
    return true;
}

__global__ __launch_bounds__(256) void lm_score_kernel(const void* tables, const int32_t* __restrict__ words,
                                                       const int64_t* __restrict__ offsets, int n, int boundary,
                                                       double* __restrict__ out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const LmView lm = lm_view(tables);
    int ctx[LM_CTX];
#pragma unroll
    for (int i = 0; i < LM_CTX; ++i) ctx[i] = -1;
    if (boundary) ctx[LM_CTX - 1] = lm.bos;
    double acc = 0.0;
    for (int64_t i = offsets[s], e = offsets[s + 1]; i < e; ++i) {
        int w = words[i];
        if (w < 0 || w >= lm.n_words) w = lm.unk;
        acc += lm_cond_log10(lm, ctx, w);
        lm_ctx_push(ctx, w);
    }
    if (boundary) acc += lm_cond_log10(lm, ctx, lm.eos);
    out[s] = acc;
}

}  // namespace

extern "C" size_t cfm_ngram_lm_pack_bytes(int order, const int64_t* ngram_counts, int n_words, int64_t word_cp_total, int V,
                                          int64_t tok_cp_total) {
    return (size_t)lm_layout(order, ngram_counts, n_words, word_cp_total, V, tok_cp_total, nullptr);
}

extern "C" int cfm_ngram_lm_pack(int order, const int64_t* ngram_counts, const int32_t* ngram_words, const float* ngram_logp,
                                 const float* ngram_backoff, int n_words, const int64_t* word_cp_offsets, const int32_t* word_cp,
                                 int bos_id, int eos_id, int unk_id, int V, const int64_t* tok_cp_offsets,
                                 const int32_t* tok_cp, const int32_t* tok_kind, void* out, size_t out_bytes) {
    CFM_REQUIRE(ngram_counts && ngram_words && ngram_logp && ngram_backoff && word_cp_offsets && tok_cp_offsets && tok_kind && out,
                CFM_ERR_NULL);
    CFM_REQUIRE(order >= 1 && order <= LM_MAX_ORDER, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE(n_words >= 1 && V >= 1, CFM_ERR_BAD_SHAPE);
    const int64_t word_cp_total = word_cp_offsets[n_words], tok_cp_total = tok_cp_offsets[V];
    CFM_REQUIRE((word_cp || word_cp_total == 0) && (tok_cp || tok_cp_total == 0), CFM_ERR_NULL);
    LmHeader h;
    const int64_t bytes = lm_layout(order, ngram_counts, n_words, word_cp_total, V, tok_cp_total, &h);
    CFM_REQUIRE(bytes > 0 && out_bytes >= (size_t)bytes, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(bos_id >= 0 && bos_id < n_words && eos_id >= 0 && eos_id < n_words && unk_id >= 0 && unk_id < n_words,
                CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(offsets_ok(word_cp_offsets, n_words, word_cp_total) && offsets_ok(tok_cp_offsets, V, tok_cp_total),
                CFM_ERR_BAD_SHAPE);
    for (int c = 0; c < V; ++c) CFM_REQUIRE(tok_kind[c] >= LM_TOK_CHARS && tok_kind[c] <= LM_TOK_SKIP, CFM_ERR_BAD_SHAPE);
    for (int64_t i = 0; i < word_cp_total; ++i) CFM_REQUIRE(word_cp[i] >= 0, CFM_ERR_BAD_SHAPE);
    for (int64_t i = 0; i < tok_cp_total; ++i) CFM_REQUIRE(tok_cp[i] >= 0, CFM_ERR_BAD_SHAPE);

    char* base = static_cast<char*>(out);
    memset(base, 0, (size_t)bytes);
    // n-gram tables
    const int32_t* ids = ngram_words;
    const float *lp = ngram_logp, *bo = ngram_backoff;
    float unk_logp = 0.f;
    for (int n = 1; n <= order; ++n) {
        int32_t* tab = reinterpret_cast<int32_t*>(base + h.gram_off[n - 1]);
        const uint32_t mask = h.gram_mask[n - 1];
        for (int64_t i = 0; i < ((int64_t)mask + 1) * LM_GRAM_SLOT; ++i) tab[i] = -1;
        for (int64_t g = 0; g < ngram_counts[n - 1]; ++g, ids += n, ++lp, ++bo) {
            for (int i = 0; i < n; ++i) CFM_REQUIRE(ids[i] >= 0 && ids[i] < n_words, CFM_ERR_BAD_SHAPE);
            uint32_t slot = (uint32_t)gram_hash(ids, n) & mask;
            for (;;) {
                int32_t* e = tab + (int64_t)slot * LM_GRAM_SLOT;
                if (e[0] == -1) {
                    for (int i = 0; i < n; ++i) e[i] = ids[i];
                    memcpy(e + 6, lp, 4);
                    memcpy(e + 7, bo, 4);
                    break;
                }
                CFM_REQUIRE(memcmp(e, ids, (size_t)n * 4) != 0, CFM_ERR_BAD_SHAPE);      // the same n-gram twice
                slot = (slot + 1u) & mask;
            }
            if (n == 1 && ids[0] == unk_id) unk_logp = *lp;
        }
    }
    // character trie
    int32_t* trie = reinterpret_cast<int32_t*>(base + h.trie_off);
    int32_t* node_word = reinterpret_cast<int32_t*>(base + h.node_word_off);
    for (int64_t i = 0; i <= (int64_t)h.trie_mask; ++i) { trie[4 * i] = -1; trie[4 * i + 1] = -1; trie[4 * i + 2] = -1; trie[4 * i + 3] = 0; }
    for (int64_t i = 0; i <= word_cp_total; ++i) node_word[i] = -1;
    int32_t n_nodes = 1;
    for (int w = 0; w < n_words; ++w) {
        if (w == bos_id || w == eos_id || w == unk_id || word_cp_offsets[w] == word_cp_offsets[w + 1]) continue;
        int32_t node = 0;
        for (int64_t i = word_cp_offsets[w]; i < word_cp_offsets[w + 1]; ++i) {
            const int32_t cp = word_cp[i];
            uint32_t slot = (uint32_t)trie_hash(node, cp) & h.trie_mask;
            for (;;) {
                int32_t* e = trie + 4 * (int64_t)slot;
                if (e[0] == -1) { e[0] = node; e[1] = cp; e[2] = n_nodes++; node = e[2]; break; }
                if (e[0] == node && e[1] == cp) { node = e[2]; break; }
                slot = (slot + 1u) & h.trie_mask;
            }
        }
        CFM_REQUIRE(node_word[node] == -1, CFM_ERR_BAD_SHAPE);                              // two words, one spelling
        node_word[node] = w;
    }
    // vocabulary tokens
    int32_t* toff = reinterpret_cast<int32_t*>(base + h.tok_off_off);
    for (int c = 0; c <= V; ++c) toff[c] = (int32_t)tok_cp_offsets[c];
    if (tok_cp_total) memcpy(base + h.tok_cp_off, tok_cp, (size_t)tok_cp_total * 4);
    memcpy(base + h.tok_kind_off, tok_kind, (size_t)V * 4);
    h.bos = bos_id;
    h.eos = eos_id;
    h.unk = unk_id;
    h.n_nodes = n_nodes;
    h.unk_logp = unk_logp;
    memcpy(base, &h, sizeof(h));
    return CFM_OK;
}

extern "C" int cfm_ngram_lm_score_f64(const void* lm_tables, const int32_t* words, const int64_t* offsets, int n_sentences,
                                      int boundary, double* out, cfm_stream_t stream) {
    CFM_REQUIRE(lm_tables && words && offsets && out, CFM_ERR_NULL);
    CFM_REQUIRE(n_sentences >= 1, CFM_ERR_BAD_SHAPE);
    hipLaunchKernelGGL(lm_score_kernel, dim3((unsigned)((n_sentences + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), lm_tables, words, offsets, n_sentences, boundary ? 1 : 0, out);
    return cfm_launch_status();
}
