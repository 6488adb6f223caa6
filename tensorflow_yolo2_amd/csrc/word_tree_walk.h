// What the walks over a word tree share (word_tree.hip: loss, statistics, head rewrite; detect_tree.hip: the walk that
// only answers): the view of the packed tables, the range cut on everything read from them, the butterfly sum and the
// entries' check of the tree arguments.  One definition of each, moved here verbatim from word_tree.hip; both files are
// compiled with -ffp-contract=off.
//
// Tables (utils/word_tree.py pack(); device memory, int32 [3 C + 2 G]): parent[C], group[C], child[C], group_offset[G],
// group_size[G].  The host cannot see their content, so every value read from them is cut into its range before it
// becomes an index (wt_span, the node checks of the walks).
#pragma once
#include "common.h"
#include "../../include/yolo2_hip.h"

// REQUIRED OF THE INCLUDING FILE: it defines, at file scope, `static int fail(int code, const char* fmt, ...)` -- printf
// style, sets y2_last_error, returns code -- before or after this include (word_tree.hip: its own, below the include;
// detect_tree.hip: data_common.h's, above it).  wt_tree_check reports through it, so that the message carries the
// entry's name in the file's own form; a file without one fails to link its own object, not silently.
static int fail(int code, const char* fmt, ...);

struct WtTables {
    const int* parent;     // [C]
    const int* group;      // [C]
    const int* child;      // [C]
    const int* goff;       // [G]
    const int* gsize;      // [G]
    int C, G, max_depth;
};

static WtTables wt_tables(const int* tables, int C, int G, int max_depth) {
    WtTables t;
    t.parent = tables; t.group = tables + C; t.child = tables + 2 * (size_t)C;
    t.goff = tables + 3 * (size_t)C; t.gsize = tables + 3 * (size_t)C + G;
    t.C = C; t.G = G; t.max_depth = max_depth;
    return t;
}

// the members [off, off + size) of group g, cut into [0, C): size 0 where g or its entries are out of range
Y2_DEV void wt_span(const WtTables& tb, int g, int& off, int& size) {
    off = 0; size = 0;
    if (g < 0 || g >= tb.G) return;
    const int o = tb.goff[g], s = tb.gsize[g];
    if (o < 0 || o >= tb.C || s <= 0) return;
    off = o; size = min(s, tb.C - o);
}

// a butterfly: every lane ends with the same bits, and the order of the additions is fixed
Y2_DEV float wt_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

static int wt_tree_check(const char* entry, const void* tables, int num_class, int G, int max_depth) {
    if (!tables) return fail(Y2_ERR_ARG, "%s: null pointer (tables)", entry);
    if (num_class < 1 || num_class > Y2_WORD_TREE_MAX_NODES)
        return fail(Y2_ERR_ARG, "%s: num_class = %d outside 1..Y2_WORD_TREE_MAX_NODES = %d", entry, num_class,
                    Y2_WORD_TREE_MAX_NODES);
    if (G < 1 || G > num_class) return fail(Y2_ERR_ARG, "%s: G = %d outside 1..num_class = %d", entry, G, num_class);
    if (max_depth < 0 || max_depth >= num_class)
        return fail(Y2_ERR_ARG, "%s: max_depth = %d outside 0..num_class - 1 = %d", entry, max_depth, num_class - 1);
    return Y2_OK;
}
