// Catalogue walk, the 16-entry exclusion walk: the seen masks of one 16-item block [cb, cb + 16) for the lane's rows
// 4q + r.  Only a block that reaches a row's next seen item loads anything: the row's 16 lanes read its next 16 seen
// entries (one coalesced load), OR-reduce their bits and advance the cursor past every entry below cb + 16 - so the
// cursors also catch up over blocks that were never asked about.  Included at the top of the includer's per-block
// lambda (select / keys_of); plain statements, no parameters (DESIGN section 31).
//   expects  c, q, cb, seen_idx, cur[4], end[4], nxt[4] (walk_seen_cursor.inc)
//   defines  unsigned msk[4]: bit i of msk[r] set = item cb + i is in the seen row of row 4q + r;  advances cur / nxt
        unsigned msk[4] = {0u, 0u, 0u, 0u};
        bool near = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) near = near || nxt[r] < cb + 16;
        if (__ballot(near)) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bool more = nxt[r] < cb + 16;                            // same in the 16 lanes of the q group
                const bool touched = more;
                while (__ballot(more)) {
                    int s = INT32_MAX;
                    if (more) {
                        const int64_t p = cur[r] + c;
                        s = p < end[r] ? seen_idx[p] : INT32_MAX;
                    }
                    const bool below = more && s < cb + 16;
                    unsigned bit = (below && s >= cb) ? 1u << (int)(s - cb) : 0u;
                    bit |= __shfl_xor(bit, 1, 64);
                    bit |= __shfl_xor(bit, 2, 64);
                    bit |= __shfl_xor(bit, 4, 64);
                    bit |= __shfl_xor(bit, 8, 64);
                    msk[r] |= bit;
                    const int adv = __popc((unsigned)(__ballot(below) >> (16 * q)) & 0xFFFFu);
                    cur[r] += adv;
                    more = more && adv == 16;                            // 16 consumed: there may be more in the block
                }
                if (touched) nxt[r] = cur[r] < end[r] ? seen_idx[cur[r]] : INT32_MAX;
            }
        }
