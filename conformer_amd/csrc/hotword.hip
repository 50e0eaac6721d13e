// Hotword boosting for the CTC beam search: the host packer of the device tables (layout in hotword.h) and a host entry
// that runs the window step and the bonus of hotword.h over token sequences, so the device logic can be checked without a
// GPU.  conformer_amd/hotwords.py calls both; the boosted search itself is in ctc_beam.hip.
#include <string.h>
#include <vector>
#include "cfm_common.h"
#include "hotword.h"

namespace {

inline int64_t hw_align(int64_t x) { return (x + 255) & ~int64_t(255); }

inline int64_t hw_capacity(int64_t count) {                 // open addressing, load factor <= 1/2
    int64_t cap = 2;
    while (cap < 2 * count) cap <<= 1;
    return cap;
}

// byte layout of the blob; 0 if the sizes are out of range
int64_t hw_layout(int n_unigrams, int64_t uni_cp_total, int n_phrases, int64_t phrase_word_total, int V, int64_t tok_cp_total,
                  HwHeader* h) {
    if (n_unigrams < 0 || n_unigrams > HW_MAX_UNIGRAMS || n_phrases < 0 || n_phrases > HW_MAX_PHRASES || V < 1) return 0;
    if (uni_cp_total < n_unigrams || uni_cp_total >= (int64_t(1) << 30) || tok_cp_total < 0 || tok_cp_total >= INT32_MAX) return 0;
    if (phrase_word_total < n_phrases || phrase_word_total > (int64_t)n_phrases * HW_MAX_WORDS) return 0;
    HwHeader hd;
    memset(&hd, 0, sizeof(hd));
    int64_t off = hw_align(sizeof(HwHeader));
    const int64_t ccap = hw_capacity(uni_cp_total), pcap = hw_capacity(phrase_word_total);
    hd.ctrie_off = off;
    hd.ctrie_mask = (uint32_t)(ccap - 1);
    off = hw_align(off + ccap * 16);
    hd.cnode_off = off;
    off = hw_align(off + (1 + uni_cp_total) * 16);
    hd.ptrie_off = off;
    hd.ptrie_mask = (uint32_t)(pcap - 1);
    off = hw_align(off + pcap * 16);
    hd.pnode_prio_off = off;
    off = hw_align(off + (1 + phrase_word_total) * 4);
    hd.tok_off_off = off;
    off = hw_align(off + ((int64_t)V + 1) * 4);
    hd.tok_cp_off = off;
    off = hw_align(off + tok_cp_total * 4);
    hd.tok_kind_off = off;
    off = hw_align(off + (int64_t)V * 4);
    hd.magic = HW_MAGIC;
    hd.V = V;
    hd.n_phrases = n_phrases;
    hd.n_unigrams = n_unigrams;
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

// insert (node, key) into a (node, key) -> child hash; returns the child, new ones numbered from `next`
int32_t hw_insert(int32_t* tab, uint32_t mask, int32_t node, int32_t key, int32_t& next) {
    for (uint32_t slot = (uint32_t)trie_hash(node, key) & mask;; slot = (slot + 1u) & mask) {
        int32_t* e = tab + 4 * (int64_t)slot;
        if (e[0] == -1) { e[0] = node; e[1] = key; e[2] = next++; return e[2]; }
        if (e[0] == node && e[1] == key) return e[2];
    }
}

}  // namespace

extern "C" size_t cfm_hotword_pack_bytes(int n_unigrams, int64_t uni_cp_total, int n_phrases, int64_t phrase_word_total, int V,
                                         int64_t tok_cp_total) {
    return (size_t)hw_layout(n_unigrams, uni_cp_total, n_phrases, phrase_word_total, V, tok_cp_total, nullptr);
}

extern "C" int cfm_hotword_pack(int n_unigrams, const int64_t* uni_cp_offsets, const int32_t* uni_cp, int n_phrases,
                                const int64_t* phrase_offsets, const int32_t* phrase_words, int V, const int64_t* tok_cp_offsets,
                                const int32_t* tok_cp, const int32_t* tok_kind, void* out, size_t out_bytes) {
    CFM_REQUIRE(uni_cp_offsets && phrase_offsets && tok_cp_offsets && tok_kind && out, CFM_ERR_NULL);
    CFM_REQUIRE(n_unigrams >= 0 && n_unigrams <= HW_MAX_UNIGRAMS && n_phrases >= 0 && n_phrases <= HW_MAX_PHRASES,
                CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE(V >= 1, CFM_ERR_BAD_SHAPE);
    const int64_t uni_cp_total = uni_cp_offsets[n_unigrams], pw_total = phrase_offsets[n_phrases], tok_cp_total = tok_cp_offsets[V];
    CFM_REQUIRE((uni_cp || uni_cp_total == 0) && (phrase_words || pw_total == 0) && (tok_cp || tok_cp_total == 0), CFM_ERR_NULL);
    HwHeader h;
    const int64_t bytes = hw_layout(n_unigrams, uni_cp_total, n_phrases, pw_total, V, tok_cp_total, &h);
    CFM_REQUIRE(bytes > 0 && out_bytes >= (size_t)bytes, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(offsets_ok(uni_cp_offsets, n_unigrams, uni_cp_total) && offsets_ok(phrase_offsets, n_phrases, pw_total) &&
                offsets_ok(tok_cp_offsets, V, tok_cp_total), CFM_ERR_BAD_SHAPE);
    for (int u = 0; u < n_unigrams; ++u) CFM_REQUIRE(uni_cp_offsets[u + 1] > uni_cp_offsets[u], CFM_ERR_BAD_SHAPE);   // no empty word
    for (int p = 0; p < n_phrases; ++p) {
        const int64_t l = phrase_offsets[p + 1] - phrase_offsets[p];
        CFM_REQUIRE(l >= 1 && l <= HW_MAX_WORDS, CFM_ERR_BAD_SHAPE);
    }
    for (int64_t i = 0; i < pw_total; ++i) CFM_REQUIRE(phrase_words[i] >= 0 && phrase_words[i] < n_unigrams, CFM_ERR_BAD_SHAPE);
    for (int c = 0; c < V; ++c) CFM_REQUIRE(tok_kind[c] >= LM_TOK_CHARS && tok_kind[c] <= LM_TOK_SKIP, CFM_ERR_BAD_SHAPE);
    for (int64_t i = 0; i < uni_cp_total; ++i) CFM_REQUIRE(uni_cp[i] >= 0, CFM_ERR_BAD_SHAPE);
    for (int64_t i = 0; i < tok_cp_total; ++i) CFM_REQUIRE(tok_cp[i] >= 0, CFM_ERR_BAD_SHAPE);

    char* base = static_cast<char*>(out);
    memset(base, 0, (size_t)bytes);
    // character trie over the unigrams, with each node's unigram, depth and shortest completion
    int32_t* ctrie = reinterpret_cast<int32_t*>(base + h.ctrie_off);
    int32_t* cnode = reinterpret_cast<int32_t*>(base + h.cnode_off);
    for (int64_t i = 0; i <= (int64_t)h.ctrie_mask; ++i) { ctrie[4 * i] = -1; ctrie[4 * i + 1] = -1; ctrie[4 * i + 2] = -1; }
    for (int64_t i = 0; i <= uni_cp_total; ++i) { cnode[4 * i] = -1; cnode[4 * i + 1] = 0; cnode[4 * i + 2] = INT32_MAX; }
    int32_t n_cnodes = 1;
    for (int u = 0; u < n_unigrams; ++u) {
        const int32_t len = (int32_t)(uni_cp_offsets[u + 1] - uni_cp_offsets[u]);
        int32_t node = 0;
        for (int64_t i = uni_cp_offsets[u]; i < uni_cp_offsets[u + 1]; ++i) {
            node = hw_insert(ctrie, h.ctrie_mask, node, uni_cp[i], n_cnodes);
            cnode[4 * node + 1] = (int32_t)(i - uni_cp_offsets[u] + 1);
            if (len < cnode[4 * node + 2]) cnode[4 * node + 2] = len;
        }
        CFM_REQUIRE(cnode[4 * node] == -1, CFM_ERR_BAD_SHAPE);                   // two unigrams, one spelling
        cnode[4 * node] = u;
    }
    // phrase trie over unigram ids, with the best priority ending at each node
    int32_t* ptrie = reinterpret_cast<int32_t*>(base + h.ptrie_off);
    int32_t* prio = reinterpret_cast<int32_t*>(base + h.pnode_prio_off);
    for (int64_t i = 0; i <= (int64_t)h.ptrie_mask; ++i) { ptrie[4 * i] = -1; ptrie[4 * i + 1] = -1; ptrie[4 * i + 2] = -1; }
    for (int64_t i = 0; i <= pw_total; ++i) prio[i] = -1;
    int32_t n_pnodes = 1;
    for (int p = 0; p < n_phrases; ++p) {
        int32_t node = 0;
        for (int64_t i = phrase_offsets[p]; i < phrase_offsets[p + 1]; ++i)
            node = hw_insert(ptrie, h.ptrie_mask, node, phrase_words[i], n_pnodes);
        if (prio[node] < 0) prio[node] = p;                                       // phrases come in priority order
    }
    // vocabulary tokens
    int32_t* toff = reinterpret_cast<int32_t*>(base + h.tok_off_off);
    for (int c = 0; c <= V; ++c) toff[c] = (int32_t)tok_cp_offsets[c];
    if (tok_cp_total) memcpy(base + h.tok_cp_off, tok_cp, (size_t)tok_cp_total * 4);
    memcpy(base + h.tok_kind_off, tok_kind, (size_t)V * 4);
    h.n_cnodes = n_cnodes;
    h.n_pnodes = n_pnodes;
    memcpy(base, &h, sizeof(h));
    return CFM_OK;
}

extern "C" int cfm_hotword_count(const void* hw_tables, const int32_t* tokens, const int64_t* offsets, int n_seqs, double weight,
                                 int32_t* counts, double* bonus, int32_t* final_counts) {
    CFM_REQUIRE(hw_tables && offsets && counts && bonus && final_counts, CFM_ERR_NULL);
    CFM_REQUIRE(n_seqs >= 1, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(__builtin_isfinite(weight), CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(static_cast<const HwHeader*>(hw_tables)->magic == HW_MAGIC, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(offsets_ok(offsets, n_seqs, offsets[n_seqs]) && (tokens || offsets[n_seqs] == 0), CFM_ERR_BAD_SHAPE);
    const HwView hw = hw_view(hw_tables);
    for (int64_t i = 0; i < offsets[n_seqs]; ++i) CFM_REQUIRE(tokens[i] >= 0 && tokens[i] < hw.V, CFM_ERR_BAD_SHAPE);
    for (int s = 0; s < n_seqs; ++s) {
        int ids[HW_WIN] = {-1, -1, -1, -1, -1, -1, -1};
        int n = 0, decided = 0, cnt = 0, node = 0;                 // node: character-trie node of p (-1: no prefix, 0: empty)
        for (int64_t i = offsets[s]; i < offsets[s + 1]; ++i) {
            const int c = tokens[i], kind = hw.tok_kind[c];
            if (kind == LM_TOK_DELIM) {
                if (node != 0) {
                    cnt = hw_push(hw, ids, n, decided, node > 0 ? hw.cnode[node].x : -1);
                    node = 0;
                }
            } else if (kind == LM_TOK_CHARS) {
                for (int q = hw.tok_off[c]; q < hw.tok_off[c + 1] && node >= 0; ++q)
                    node = hw_child(hw.ctrie, hw.ctrie_mask, node, hw.tok_cp[q]);
            }
            counts[i] = cnt;
            bonus[i] = hw_bonus(hw, node, weight);
        }
        final_counts[s] = node != 0 ? hw_push(hw, ids, n, decided, node > 0 ? hw.cnode[node].x : -1) : cnt;
    }
    return CFM_OK;
}
