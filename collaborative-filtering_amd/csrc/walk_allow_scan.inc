// Catalogue walk, the slice's chunk count and the allow-bitmap scan of the MASKED instantiations: slices start at
// multiples of 32, so chunk ch of the slice is word lo / 32 + ch of the bitmap, and every wave finds the next chunk
// with a set bit by the same scan (64 words per step: one per lane, ballot, count trailing zeros) - the workgroup's
// barriers stay matched.  Included in the kernel body in front of the chunk loop; plain statements, no parameters
// (DESIGN section 31).  An unmasked instantiation never calls the lambdas and contains none of them.
//   expects  lane, lo, hi, allow, MASKED
//   defines  nch (chunks of the slice), aw, next_chunk(ch), pw, window(from), after(ch)
    const int64_t nch = hi > lo ? (hi - lo + walk::CHUNK - 1) / walk::CHUNK : 0;
    const uint32_t* aw = MASKED ? allow + lo / walk::CHUNK : nullptr;   // word of chunk 0 (lo is a multiple of 32)
    // first chunk >= ch with an allowed item, nch if there is none: the same value in every wave of the workgroup
    auto next_chunk = [&](int64_t ch) -> int64_t {
        for (; ch < nch; ch += 64) {
            const unsigned w = ch + lane < nch ? aw[ch + lane] : 0u;
            const unsigned long long m = __ballot(w != 0u);
            if (m) return ch + __builtin_ctzll(m);
        }
        return nch;
    };
    // the scan is kept off the prefetch's path: while chunk ch is scored, this lane's word of the window
    // [ch + 1, ch + 65) is in flight behind the Z loads, and the chunk after ch is read off it by one ballot
    unsigned pw = 0u;
    auto window = [&](int64_t from) { pw = from + lane < nch ? aw[from + lane] : 0u; };
    auto after = [&](int64_t ch) -> int64_t {
        const unsigned long long m = __ballot(pw != 0u);
        return m ? ch + 1 + __builtin_ctzll(m) : next_chunk(ch + 65);
    };
