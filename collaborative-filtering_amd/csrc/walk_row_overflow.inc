// Catalogue walk, end of a chunk for the lambda-form row state (walk_row_lists.inc): every row whose buffer could
// overflow in the next chunk of walk::CHUNK candidates is compacted.  Included at the end of the chunk loop's body;
// plain statements, no parameters (DESIGN section 31).
//   expects  cnt[4], compact(r), readlane_i, BUF
        bool full = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) full = full || cnt[r] > BUF - walk::CHUNK;
        if (__ballot(full)) {                            // some row's buffer could overflow in the next chunk
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_wave_barrier();
            for (int r = 0; r < 16; ++r) {
                int rc = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) rc = ((r & 3) == e) ? cnt[e] : rc;
                rc = readlane_i(rc, 16 * (r >> 2));
                if (rc > BUF - walk::CHUNK) compact(r);
            }
        }
