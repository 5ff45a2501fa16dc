// qr_split.h — the index split of a quotient-remainder table, shared by emb_qr.hip and interact_qr.hip (include after common.h).
#pragma once

// the reference's index split: q = (int64)((float)id / (float)c) — a FLOAT32 division (see emb_qr.hip) — and r = id mod c.
// false: the lookup names no row (skipped and reported by the caller)
__device__ __forceinline__ bool qr_split(long long id, long long n, int c, long long rows_q, long long* q, long long* r) {
    if (!dlrm_index_ok(id, n)) return false;
    const long long qq = (long long)__fdiv_rn((float)id, (float)c);
    if (!dlrm_index_ok(qq, rows_q)) return false;
    *q = qq; *r = id % c;
    return true;
}
