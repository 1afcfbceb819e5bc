// Catalogue walk, seen-cursor set-up of one row 4q + r: where the row's ascending seen list enters the slice [lo, hi).
// Included inside the includer's `for (int r = 0; r < 4; ++r)`; plain statements, no parameters (DESIGN section 31).
//   expects  r, u (the row's user id: k_rank_count aliases it to su[r]), valid[4], lo, seen_ptr, seen_idx,
//            and the declared arrays int64_t cur[4], end[4]; int nxt[4]
//   sets     cur[r] (first entry >= lo), end[r], nxt[r] (the item at cur[r], INT32_MAX when the list is used up)
        cur[r] = end[r] = 0;
        if (seen_ptr && valid[r]) {
            int64_t a = seen_ptr[u], e = seen_ptr[u + 1];
            end[r] = e;
            while (a < e) {                                              // first seen item >= lo
                const int64_t mid = a + ((e - a) >> 1);
                if (seen_idx[mid] < lo) a = mid + 1; else e = mid;
            }
            cur[r] = a;
        }
        nxt[r] = cur[r] < end[r] ? seen_idx[cur[r]] : INT32_MAX;
