// Catalogue walk, Z staging: the rows walk_z_fetch.inc left in registers go to the workgroup's LDS tile, between the
// two barriers of the chunk loop.  The body of the includer's `stage` lambda; plain statements, no parameters (DESIGN
// section 31).
//   expects  tid, f32x4 pf[PF], zs[walk::CHUNK][ZS], and the constants LD, NT, NV, PF of walk_z_fetch.inc
//   sets     zs[i][0 .. LD) for the CHUNK rows i
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int v = tid + p * NT;
            if (v < NV) {
                const int i = v / (LD / 4), d = v - i * (LD / 4);
                *reinterpret_cast<f32x4*>(&zs[i][4 * d]) = pf[p];
            }
        }
