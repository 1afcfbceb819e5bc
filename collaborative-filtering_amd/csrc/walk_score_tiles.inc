// Catalogue walk, the two 16 x 16 score tiles of a staged chunk: the SAME v_mfma_f32_16x16x4_f32 chain as
// k_predict_dense - lane (c, q) holds k = 4KB q + e of operand row c and of item row c in step e - so with walk::score
// every score is bitwise the value als_predict_dense writes.  Included in the chunk loop behind the staging barriers;
// plain statements, no parameters (DESIGN section 31).
//   expects  c, q, ua[E] (the wave's 16 operand rows in that layout), zs, E
//   defines  z0[E], z1[E], f32x4 acc0 (items it0 ... it0 + 15), acc1 (items it0 + 16 ... it0 + 31)
        float z0[E], z1[E];
        load_frow<E>(&zs[c][E * q], z0);
        load_frow<E>(&zs[16 + c][E * q], z1);
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < E; ++e) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[e], z0[e], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[e], z1[e], acc1, 0, 0, 0);
        }
