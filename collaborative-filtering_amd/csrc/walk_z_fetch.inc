// Catalogue walk, Z prefetch: the workgroup's NT threads load the LD floats of the walk::CHUNK item rows from it0 on
// into registers (rows past the catalogue repeat row n - 1), so the global loads of the next chunk are in flight while
// the current one is scored; walk_z_stage.inc stores them to LDS.  The body of the includer's `fetch` lambda - a kernel
// with per-chunk data of its own (k_priced: the floors) adds its lines behind the include; plain statements, no
// parameters (DESIGN section 31).
//   expects  it0, tid, n, ld, Z, f32x4 pf[PF], and the constants LD, NT, NV = walk::CHUNK * LD / 4, PF = ceil(NV / NT)
//   sets     pf[0 .. PF)
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int v = tid + p * NT;
            if (v < NV) {
                const int i = v / (LD / 4), d = v - i * (LD / 4);
                pf[p] = *reinterpret_cast<const f32x4*>(Z + (size_t)min(it0 + i, n - 1) * ld + 4 * d);
            }
        }
