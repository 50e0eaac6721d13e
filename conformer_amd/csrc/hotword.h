// Hotword tables for CTC beam-search boosting ("Hotword boosting"): the layout of the packed blob, the
// lookups, and the two pieces of the scoring the device search (ctc_beam.hip) and the host entry cfm_hotword_count
// (hotword.hip) share: the window step that keeps a hypothesis's match count, and the partial-word bonus Q.
//
// The blob (one allocation, every section 256-byte aligned, offsets in bytes from its start):
//   HwHeader
//   ctrie: the character trie over the spellings of the hotword unigrams, as a (node, code point) -> child hash (trie_hash of
//       ngram_lm.h): (ctrie_mask + 1) int4 slots (node, code point, child, 0), node == -1: empty slot.  Node 0 is the root.
//   cnode: int4 per character-trie node: (unigram id whose spelling ends there or -1, depth in code points, the length of
//       the shortest unigram that has the node's spelling as a prefix, 0).
//   ptrie: the word-level phrase trie over unigram ids, the same hash: (ptrie_mask + 1) int4 slots (node, unigram id, child,
//       0).  Node 0 is the root.
//   pnode_prio: int32 per phrase-trie node: the best (lowest) priority of a phrase that ends there, or -1.
//   tok_off (V + 1 int32), tok_cp, tok_kind (V int32): the vocabulary tokens, as in the LM blob (LM_TOK_*).
//
// Counting (the window rule).  count(words) is the number of phrases a left-to-right scan finds when, at each word, it takes
// the first phrase in priority order that matches there and jumps past it (one word on if none matches).  A decision at a
// word depends on at most HW_MAX_WORDS words, so a hypothesis keeps only the matches already decided and a window of the
// (at most HW_WIN) undecided words: a completed word is appended, and while the window holds HW_MAX_WORDS words the
// decision at its first word is taken.  count = decided + the scan over the window read as the end of the text.
#pragma once
#include "ngram_lm.h"

constexpr uint32_t HW_MAGIC = 0x57484643u;           // "CFHW"
constexpr int HW_MAX_WORDS = 8;                      // words per phrase
constexpr int HW_WIN = HW_MAX_WORDS - 1;             // undecided words a hypothesis carries
constexpr int HW_MAX_PHRASES = 1024;
constexpr int HW_MAX_UNIGRAMS = HW_MAX_PHRASES * HW_MAX_WORDS;   // unigram ids fit int16

struct HwHeader {
    uint32_t magic;
    int32_t V, n_phrases, n_unigrams, n_cnodes, n_pnodes;
    int64_t total_bytes;
    int64_t ctrie_off, cnode_off, ptrie_off, pnode_prio_off, tok_off_off, tok_cp_off, tok_kind_off;
    uint32_t ctrie_mask, ptrie_mask;
};

struct HwView {
    const int4 *ctrie, *cnode, *ptrie;
    const int32_t *pnode_prio, *tok_off, *tok_cp, *tok_kind;
    uint32_t ctrie_mask, ptrie_mask;
    int V;
};

CFM_HD HwView hw_view(const void* tables) {
    const char* base = static_cast<const char*>(tables);
    const HwHeader* h = static_cast<const HwHeader*>(tables);
    HwView v;
    v.ctrie = reinterpret_cast<const int4*>(base + h->ctrie_off);
    v.cnode = reinterpret_cast<const int4*>(base + h->cnode_off);
    v.ptrie = reinterpret_cast<const int4*>(base + h->ptrie_off);
    v.pnode_prio = reinterpret_cast<const int32_t*>(base + h->pnode_prio_off);
    v.tok_off = reinterpret_cast<const int32_t*>(base + h->tok_off_off);
    v.tok_cp = reinterpret_cast<const int32_t*>(base + h->tok_cp_off);
    v.tok_kind = reinterpret_cast<const int32_t*>(base + h->tok_kind_off);
    v.ctrie_mask = h->ctrie_mask;
    v.ptrie_mask = h->ptrie_mask;
    v.V = h->V;
    return v;
}

// child of `node` by `key` in a (node, key) -> child hash, or -1
CFM_HD int hw_child(const int4* tab, uint32_t mask, int node, int key) {
    for (uint32_t slot = (uint32_t)trie_hash(node, key) & mask;; slot = (slot + 1u) & mask) {
        const int4 e = tab[slot];
        if (e.x == -1) return -1;
        if (e.x == node && e.y == key) return e.z;
    }
}

// Q(p) for the partial word at character-trie node `node` (-1: p is no prefix of a unigram, 0: p is empty): weight * len(p)
// / (the length of the shortest unigram with prefix p), in fp64 in that order; 0 where p is empty or no hotword prefix
CFM_HD double hw_bonus(const HwView& hw, int node, double weight) {
    if (node <= 0) return 0.0;
    const int4 e = hw.cnode[node];
    return weight * (double)e.y / (double)e.z;
}

// length in words of the first phrase in priority order that matches w[I..n) at I (0: none)
template <int I>
CFM_HD int hw_match(const HwView& hw, const int (&w)[HW_MAX_WORDS], int n) {
    int node = 0, best = INT32_MAX, len = 0;
#pragma unroll
    for (int j = I; j < HW_MAX_WORDS; ++j) {
        if (j >= n || w[j] < 0) break;
        node = hw_child(hw.ptrie, hw.ptrie_mask, node, w[j]);
        if (node < 0) break;
        const int pr = hw.pnode_prio[node];
        if (pr >= 0 && pr < best) { best = pr; len = j - I + 1; }
    }
    return len;
}

template <int I>
CFM_HD void hw_match_all(const HwView& hw, const int (&w)[HW_MAX_WORDS], int n, int (&len)[HW_MAX_WORDS]) {
    if constexpr (I < HW_MAX_WORDS) {
        len[I] = I < n ? hw_match<I>(hw, w, n) : 0;
        hw_match_all<I + 1>(hw, w, n, len);
    }
}

// matches of the scan over w[0..n) read as the end of the text (every index a constant: the arrays stay in registers)
CFM_HD int hw_scan(const HwView& hw, const int (&w)[HW_MAX_WORDS], int n) {
    int len[HW_MAX_WORDS];
    hw_match_all<0>(hw, w, n, len);
    int c = 0, next = 0;
#pragma unroll
    for (int i = 0; i < HW_MAX_WORDS; ++i) {
        if (i == next && i < n) {
            if (len[i]) { ++c; next = i + len[i]; } else { next = i + 1; }
        }
    }
    return c;
}

// The window step: append the completed word `uid` (its unigram id, or -1) to the window ids[0..n) of a hypothesis with
// `decided` matches, decide at the first word if the window then holds HW_MAX_WORDS words, and return the new count.
CFM_HD int hw_push(const HwView& hw, int (&ids)[HW_WIN], int& n, int& decided, int uid) {
    int w[HW_MAX_WORDS];
#pragma unroll
    for (int i = 0; i < HW_MAX_WORDS; ++i) w[i] = i < HW_WIN && i < n ? ids[i] : (i == n ? uid : -1);
    int m = n + 1, drop = 0;
    if (m == HW_MAX_WORDS) {
        const int l = hw_match<0>(hw, w, m);
        if (l) ++decided;
        drop = l ? l : 1;
    }
    m -= drop;
#pragma unroll
    for (int i = 0; i < HW_WIN; ++i) {
        int x = w[i];
#pragma unroll
        for (int d = 1; d < HW_MAX_WORDS; ++d)
            if (drop == d) x = i + d < HW_MAX_WORDS ? w[i + d] : -1;
        if (drop == HW_MAX_WORDS) x = -1;
        ids[i] = i < m ? x : -1;
    }
    n = m;
    int r[HW_MAX_WORDS];
#pragma unroll
    for (int i = 0; i < HW_MAX_WORDS; ++i) r[i] = i < HW_WIN ? ids[i] : -1;
    return decided + hw_scan(hw, r, n);
}

// count of the window ids[0..n) with `decided` matches already taken
CFM_HD int hw_count(const HwView& hw, const int (&ids)[HW_WIN], int n, int decided) {
    int r[HW_MAX_WORDS];
#pragma unroll
    for (int i = 0; i < HW_MAX_WORDS; ++i) r[i] = i < HW_WIN ? ids[i] : -1;
    return decided + hw_scan(hw, r, n);
}
