// attn_check.h — host only: the geometry rules of PncAttnParams that pnc_attn_views_f16 (attn.hip) and pnc_attn_views_split_f16
// (attn_split.hip) share, each written once; a breach is PNC_EINVAL at either entry point.  An entry point keeps what is its own:
// pointers and alignment, segment ids (halo views), `causal`, H / kvH / kv_rows_per_group on the split path.  Three predicates, not
// one, so that each entry point asks them in the order its checks always had (attn.hip looks at alignment after the first).
#pragma once
#include "panacea_hip.h"

namespace pnc_attn {
// 1 .. 8 views on either side, each a whole number of columns.  The rules below divide by the view counts: ask this one first.
inline bool views_ok(const PncAttnParams& p) {
    return p.views >= 1 && p.views <= 8 && p.kv_views >= 1 && p.kv_views <= 8 && p.W % p.views == 0 && p.kvW % p.kv_views == 0;
}
// query groups per key group, groups, heads; the valid keys of a view lie inside it (kvH rows of kvW / kv_views columns)
inline bool counts_ok(const PncAttnParams& p) {
    return p.q_per_kv >= 1 && p.groups >= 1 && p.heads >= 1 && p.kv_valid >= 1 && p.kv_valid <= p.kvH * (p.kvW / p.kv_views);
}
// one or two key segments for query view v
inline bool nseg_ok(const PncAttnParams& p, int v) { return p.nseg[v] >= 1 && p.nseg[v] <= 2; }
}  // namespace pnc_attn
