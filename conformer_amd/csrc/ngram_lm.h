// Word n-gram language model tables for CTC beam-search fusion ("Language-model fusion"): the layout of the
// packed blob, the ONE hash function the host packer (ngram_lm.hip) and the device lookups share, and the device lookups.
//
// The blob (one allocation, every section 256-byte aligned, offsets in bytes from its start):
//   LmHeader
//   gram[n-1], n = 1..order: open-addressing table of the n-grams, (gram_mask[n-1] + 1) slots of LM_GRAM_SLOT int32:
//       ids[0..n) (ids[0] == -1: empty slot), unused ids -1, then float log10 p, float log10 backoff at [6], [7].
//       Keyed by gram_hash of the exact id tuple, linear probing, load factor <= 1/2; a hit is confirmed on all n ids.
//   trie: the character trie over the spellings of the unigrams (without <s>, </s>, <unk>), as a (node, code point) -> child
//       hash: (trie_mask + 1) int4 slots (node, code point, child, 0), node == -1: empty slot.  Node 0 is the root.
//   node_word: int32 per trie node, the word id whose spelling ends there, or -1.
//   tok_off (V + 1 int32), tok_cp: CSR list of the code points of each vocabulary token; tok_kind (V int32): LM_TOK_*.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CFM_HD __host__ __device__ __forceinline__

constexpr uint32_t LM_MAGIC = 0x4D4C4643u;          // "CFLM"
constexpr int LM_MAX_ORDER = 6;
constexpr int LM_CTX = LM_MAX_ORDER - 1;            // context words a hypothesis carries
constexpr int LM_GRAM_SLOT = 8;                     // int32 per n-gram slot (32 bytes, two int4 loads)
constexpr int LM_TOK_CHARS = 0, LM_TOK_DELIM = 1, LM_TOK_SKIP = 2;

struct LmHeader {
    uint32_t magic;
    int32_t order, V, n_words, bos, eos, unk, n_nodes;
    float unk_logp;                                  // log10 p(<unk>)
    int32_t pad0;
    int64_t total_bytes;
    int64_t gram_off[LM_MAX_ORDER];
    uint32_t gram_mask[LM_MAX_ORDER];
    int64_t trie_off, node_word_off, tok_off_off, tok_cp_off, tok_kind_off;
    uint32_t trie_mask, pad1;
};

CFM_HD uint64_t lm_mix(uint64_t h, uint32_t x) {
    uint64_t z = h + (uint64_t)(x + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// hash of the n-gram ids[0..n)
CFM_HD uint64_t gram_hash(const int32_t* ids, int n) {
    uint64_t h = 0x6A09E667F3BCC909ull + (uint64_t)n;
    for (int i = 0; i < n; ++i) h = lm_mix(h, (uint32_t)ids[i]);
    return h;
}
// hash of the trie edge (node, code point)
CFM_HD uint64_t trie_hash(int32_t node, int32_t cp) { return lm_mix(lm_mix(0xBB67AE8584CAA73Bull, (uint32_t)node), (uint32_t)cp); }

struct LmView {
    const int4* gram[LM_MAX_ORDER];
    uint32_t gram_mask[LM_MAX_ORDER];
    const int4* trie;
    uint32_t trie_mask;
    const int32_t *node_word, *tok_off, *tok_cp, *tok_kind;
    int order, V, n_words, bos, eos, unk;
    float unk_logp;
};

__device__ __forceinline__ LmView lm_view(const void* tables) {
    const char* base = static_cast<const char*>(tables);
    const LmHeader* h = static_cast<const LmHeader*>(tables);
    LmView v;
#pragma unroll
    for (int n = 0; n < LM_MAX_ORDER; ++n) {
        v.gram[n] = reinterpret_cast<const int4*>(base + h->gram_off[n]);
        v.gram_mask[n] = h->gram_mask[n];
    }
    v.trie = reinterpret_cast<const int4*>(base + h->trie_off);
    v.trie_mask = h->trie_mask;
    v.node_word = reinterpret_cast<const int32_t*>(base + h->node_word_off);
    v.tok_off = reinterpret_cast<const int32_t*>(base + h->tok_off_off);
    v.tok_cp = reinterpret_cast<const int32_t*>(base + h->tok_cp_off);
    v.tok_kind = reinterpret_cast<const int32_t*>(base + h->tok_kind_off);
    v.order = h->order; v.V = h->V; v.n_words = h->n_words;
    v.bos = h->bos; v.eos = h->eos; v.unk = h->unk;
    v.unk_logp = h->unk_logp;
    return v;
}

// log10 P(w | ctx) by ARPA backoff.  ctx[0..LM_CTX) holds the context words oldest first, left-padded with -1; w is a word id
// of the model (OOV words are passed as <unk>).  With x = ctx ++ [w] and c the number of usable context words
// (min(order - 1, trailing valid words)), the probes of every n-gram x[5-j..5] (j = 0..c) and every context x[5-j..4]
// (j = 1..c) are independent: they advance together, one slot per round, so their loads are in flight at the same time.
// The result is p(x[5-j..5]) + sum over j' in (j, c] of bo(x[5-j'..4]) for the largest present j; absent contexts add 0.
__device__ __forceinline__ double lm_cond_log10(const LmView& lm, const int (&ctx)[LM_CTX], int w) {
    int x[LM_CTX + 1];
#pragma unroll
    for (int i = 0; i < LM_CTX; ++i) x[i] = ctx[i];
    x[LM_CTX] = w;
    int c = 0;
#pragma unroll
    for (int i = LM_CTX - 1; i >= 0; --i)
        if (c == LM_CTX - 1 - i && x[i] >= 0 && c < lm.order - 1) ++c;
    // probe q < 6: the n-gram of context length j = q (n = q + 1); probe q >= 6: the context of length j = q - 5 (n = j)
    constexpr int NP = 2 * LM_MAX_ORDER - 1;
    bool act[NP], hit[NP];
    uint32_t slot[NP];
    float val[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int j = q < LM_MAX_ORDER ? q : q - (LM_MAX_ORDER - 1);
        const int n = q < LM_MAX_ORDER ? j + 1 : j;
        const int first = LM_CTX - j;                                     // ids x[first .. first + n)
        act[q] = j <= c;
        hit[q] = false;
        val[q] = 0.f;
        slot[q] = 0u;
        if (act[q]) {
            int32_t ids[LM_MAX_ORDER];
#pragma unroll
            for (int i = 0; i < LM_MAX_ORDER; ++i) ids[i] = i < n ? x[first + i] : -1;
            slot[q] = (uint32_t)gram_hash(ids, n) & lm.gram_mask[n - 1];
        }
    }
    for (;;) {
        bool any = false;
#pragma unroll
        for (int q = 0; q < NP; ++q) any |= act[q];
        if (!any) break;
        int4 a[NP], b[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int n = q < LM_MAX_ORDER ? q + 1 : q - (LM_MAX_ORDER - 1);
            if (act[q]) {
                const int4* s = lm.gram[n - 1] + 2 * (size_t)slot[q];
                a[q] = s[0];
                b[q] = s[1];
            }
        }
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int j = q < LM_MAX_ORDER ? q : q - (LM_MAX_ORDER - 1);
            const int n = q < LM_MAX_ORDER ? j + 1 : j;
            const int first = LM_CTX - j;
            if (!act[q]) continue;
            if (a[q].x == -1) { act[q] = false; continue; }
            const int32_t e[LM_GRAM_SLOT - 2] = {a[q].x, a[q].y, a[q].z, a[q].w, b[q].x, b[q].y};
            bool eq = true;
#pragma unroll
            for (int i = 0; i < LM_MAX_ORDER; ++i)
                if (i < n) eq = eq && e[i] == x[first + i];
            if (eq) {
                act[q] = false;
                hit[q] = true;
                val[q] = q < LM_MAX_ORDER ? __int_as_float(b[q].z) : __int_as_float(b[q].w);
            } else {
                slot[q] = (slot[q] + 1u) & lm.gram_mask[n - 1];
            }
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int j = LM_MAX_ORDER - 1; j >= 0; --j) {
        if (j > c) continue;
        if (hit[j]) return acc + (double)val[j];
        if (j >= 1 && hit[LM_MAX_ORDER - 1 + j]) acc += (double)val[LM_MAX_ORDER - 1 + j];
    }
    return acc + (double)lm.unk_logp;               // not reached: every word id has a unigram
}

// context after the word w: shift left, append
__device__ __forceinline__ void lm_ctx_push(int (&ctx)[LM_CTX], int w) {
#pragma unroll
    for (int i = 0; i < LM_CTX - 1; ++i) ctx[i] = ctx[i + 1];
    ctx[LM_CTX - 1] = w;
}
