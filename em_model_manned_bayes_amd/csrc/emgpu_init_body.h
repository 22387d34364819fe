// emgpu_init_body.h -- the attempt loop of the initial network, as text: initial network + dediscretize + rejection loop, shared by every
// DBN kernel through the four init_network forms of emgpu_device.h, which include it as their body.
// bn_sample.m:39-57, dbn_hierarchical_sample.m:25-31, UncorEncounterModel.m:248-281.
// The including function supplies NI, the run A, rng, bin[NI] (0-based bins by topological position), val[NI] (dediscretised f64),
// attempts_used = -1, no_dedisc (EMGPU_FLAG_NO_DEDISC) and
//   EMGPU_INIT_P(f)           the plan's entry f
//   EMGPU_INIT_FRESH_PLAN     what an attempt does to the plan before it reads it (nothing, or launder the kernel-argument pointer)
//   EMGPU_INIT_PRESET(p)      a declaration of `preset`: the preset bin (1-based) of the node at position p, or 0
// The loop leaves attempts_used at the number of attempts used (>= 1), or at -1 when max_attempts was reached, and rng.attempt at the
// accepted attempt.  Text and not a function template with the plan and the presets as policies: these kernels are tuned to the register,
// and every template form tried moved the allocator (HISTORY.md section 32: scratch in k_dbn_step<16,4,8>, a register in
// k_dbn_step<9,3,8,lds,ct>), while the text compiles to what the four written-out copies did.  For the same reason the two declarations
// stay ahead of a form's preset set-up, and `preset` is a value where the copy read the preset once and a reference where it read it at
// each use.
    for (uint32_t attempt = 0; attempt < (uint32_t)A.max_attempts; attempt++) {
        EMGPU_INIT_FRESH_PLAN
        rng.attempt = attempt;
        uint4 wc = make_uint4(0, 0, 0, 0);
        int wblk = -1;
#pragma unroll
        for (int p = 0; p < NI; p++) {
            EMGPU_INIT_PRESET(p)
            if (p < EMGPU_INIT_P(ni) && preset != 0) { // bn_sample.m:44-50
                bin[p] = (int)preset - 1;
            } else if (p < EMGPU_INIT_P(ni)) {
                uint32_t col = 0; // asub2ind.m:13-14 as strides
#pragma unroll
                for (int q = 0; q < p; q++) col += EMGPU_INIT_P(i_stride[p][q]) * (uint32_t)bin[q];
                const int r = EMGPU_INIT_P(i_r[p]);
                const int var = EMGPU_INIT_P(i_var[p]);
                if ((var >> 2) != wblk) { wblk = var >> 2; wc = rng.block(EMGPU_SEC_INIT, 0u, (uint32_t)wblk); }
                bin[p] = draw_bin(EMGPU_INIT_P(thr) + EMGPU_INIT_P(i_off[p]) + (size_t)col * (uint32_t)(r - 1), r, word_of(wc, var & 3)); // bn_sample.m:55
            }
        }
        // dbn_hierarchical_sample.m:25-31
        wblk = -1;
#pragma unroll
        for (int p = 0; p < NI; p++) {
            double v = (double)(bin[p] + 1);
            if (p < EMGPU_INIT_P(ni) && !no_dedisc && EMGPU_INIT_P(i_nb[p]) != 0 && !EMGPU_INIT_P(i_skip[p])) {
                const int var = EMGPU_INIT_P(i_var[p]);
                if ((var >> 2) != wblk) { wblk = var >> 2; wc = rng.block(EMGPU_SEC_DEDISC_INIT, 0u, (uint32_t)wblk); }
                v = (EMGPU_INIT_P(i_zero[p]) == bin[p] + 1) ? 0.0 : dedisc_f64(EMGPU_INIT_P(bnd), EMGPU_INIT_P(i_boff[p]), bin[p], word_of(wc, var & 3));
            }
            val[p] = v;
        }
        // UncorEncounterModel.m:259-272
        if (A.pos_L >= 0 && (A.layers != nullptr || (A.flags & EMGPU_FLAG_QUANTIZE500))) {
            double h_ft = pick<NI>(val, A.pos_L);
            if (A.layers != nullptr) {
                int b = (int)h_ft;
                b = b < 1 ? 1 : (b > A.n_layers ? A.n_layers : b);
                const double lo = A.layers[2 * (b - 1)], hi = A.layers[2 * (b - 1) + 1];
                const uint4 wl = rng.block(EMGPU_SEC_LAYER, 0u, 0u);
                {
#pragma clang fp contract(off)
                    const double d = hi - lo;
                    const double m = uniform32(wl.x) * d;
                    h_ft = lo + m;
                }
            }
            if ((A.flags & EMGPU_FLAG_QUANTIZE500) && A.pos_dh >= 0 && pick<NI>(val, A.pos_dh) == 0.0) h_ft = round500(h_ft);
            put<NI>(val, A.pos_L, h_ft);
        }
        bool good = true;
        if (A.pos_v >= 0 && A.pos_dh >= 0) { // :275
#pragma clang fp contract(off)
            const double lhs = pick<NI>(val, A.pos_v) * 1.68781;
            const double rhs = fabs(pick<NI>(val, A.pos_dh)) / 60.0;
            good = lhs > rhs;
        }
        if (good) { attempts_used = (int32_t)attempt + 1; break; }
    }
