// ct_rollout_sync_body.h -- the body of the step-synchronous rollout kernels (the ct_rollout_*.hip files; ct_rollout_sync.hip.h
// says which family lives where), included once per kernel:
// ct_rollout_sync_kernel (actions staged by the caller), ct_rollout_policy (actions drawn in the kernel), ct_rollout_pstats
// (drawn in the kernel, the transitions tallied instead of stored) and their episodic forms ct_rollout_policy_ep /
// ct_rollout_pstats_ep / ct_rollout_sync_ep (an env that ends an episode is reset inside the launch), ct_rollout_pop_ep, and the
// scored ct_rollout_policy_eps / ct_rollout_pop_eps / ct_rollout_sync_eps, ct_rollout_backlog and ct_rollout_backlog_pop.  It is text
// with macro hooks, not a function, on purpose.  As a __forceinline__ template over an action-source type the compiler
// optimised the callee on its own before inlining it, and all 30 instantiations of ct_rollout_sync_kernel came out different
// (up to 31 more VGPRs at D = 16 and 32, SGPRs parked in VGPR lanes at D = 4); with the source as an object whose members hold
// the action pointers, 28 still differed in instruction order.  Included, with the staged source's statements spelled as they
// were, every one of them is instruction for instruction what it was.
// The including kernel provides: template parameters DT and MODE; st (GwState), c (GwDevConst), K; and
//   GW_ROLLOUT_SRC_STAGE            statements before the block's barrier (tables of the source's own -> LDS)
//   GW_ROLLOUT_SRC_FIRST            statements once per lane, before step 0
//   GW_ROLLOUT_SRC_TAKE             statements at the start of step k that define `const int d, du`, the step's action
//   GW_ROLLOUT_SRC_CHECKED(bad)     `bad` if an action can lie outside the action space, else false
//                                   (ct_rollout_sync.hip.h spells both pairs once: GW_ROLLOUT_STAGED_* and GW_ROLLOUT_DRAWN_*)
//   GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)   the last statements of step k (index `at` of [K][N] outputs; k not yet
//                                   advanced): its outcome where the kernel wants it -- GW_ROLLOUT_STORE_OUTPUTS, the three
//                                   stores into the kernel's obs, reward and done, or a tally -- then the action taken, the
//                                   next draw, the episodic kernels' bookkeeping (ended[at]).  An includer that defines
//                                   GW_ROLLOUT_SRC_RESETS may call reset_env() here: gw_reset for this one env, in registers
//                                   (see there).  Such a kernel stores the env's `ip` record behind the body
//                                   (GW_ROLLOUT_EP_TAIL), which no other does.  An includer that defines
//                                   GW_ROLLOUT_SRC_QUEUES may call queues_now() in GW_ROLLOUT_SRC_TAKE and then read the body's
//                                   len[0 .. D): every queue's length at the env's current time (ct_rollout_backlog).
// The hooks share the body's scope.  Of its names they read only e, N, k, K, c and -- the scored kernels' STEPPED, for the
// packets a step delivered -- the running kt.deliv, which restarts at 0 in every launch; they define only d and du; whatever else a
// source keeps lives in names the body leaves free: `src` and anything ending in `_next`.  A new local of the body takes
// neither form.  The hooks are one include's: the body's last lines undefine all of them, so an includer defines and never
// undefines.
    // Actions and outputs in the C-ABI's own step-major layout ([K][N]: a step's row is coalesced across the wave's lanes), read
    // and written by this kernel itself: step k + 1's action is loaded while step k is walked, a step's three outputs are
    // stores nothing waits for.  (The event loop reads packed per-env action records and writes feedback bytes, with a
    // transposing kernel on either side: 15 us per 64 steps x 65 536 envs, an eighth of this kernel's own time.)
    constexpr bool GEN = DT == 0;                        // any sender count: per-lane arrays in LDS columns (as in the event loop)
    constexpr int DM = GEN ? GW_MAX_DEVICES : DT;        // capacity
    constexpr int NWC = (2 * DM + 1 + 15) / 16;
    constexpr int S = GW_MAX_NSTATES;
    const int D = GEN ? c.D : DT, R = D + 1, RRM = D;
    const uint32_t N = (uint32_t)st.N;
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;

    constexpr int TRANS_B = ((DM + 1) * (DM + 1) * S + 15) / 16 * 16;
    __shared__ __attribute__((aligned(16))) uint8_t s_trans[TRANS_B];
    __shared__ __attribute__((aligned(16))) double  s_ber[2 * DM * S];
    __shared__ __attribute__((aligned(16))) uint8_t s_cls[2 * DM * S];
    __shared__ uint32_t s_cols[GEN ? (3 * DM + 1) * 64 : 1];     // GEN: len[D], tb[D], sta[R] columns per lane
    __shared__ uint2 s_mi[GEN ? DM : 1];                 // GEN: {mult, ceil(65536/mult)} and terminal-state masks, indexed by
    __shared__ uint32_t s_term[GEN ? DM : 1];            //      the lane's own addressed sender
    if constexpr (GEN) {
        for (int i = threadIdx.x; i < D; i += blockDim.x) {
            s_mi[i] = make_uint2((uint32_t)st.cst->mult[i], st.cst->inv16[i]);
            s_term[i] = st.cst->term[i];
        }
    }
    {
        const int n_tr = (R * R * S + 15) >> 4, n_be = (2 * D * S * 8) >> 4, n_cl = (2 * D * S) >> 4;
        for (int i = threadIdx.x; i < n_tr; i += blockDim.x) *reinterpret_cast<uint4*>(s_trans + ((uint32_t)i << 4)) = ld<uint4>(st.trans, (uint32_t)i << 4);
        for (int i = threadIdx.x; i < n_be; i += blockDim.x) *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(s_ber) + ((uint32_t)i << 4)) = ld<uint4>(st.ber2, (uint32_t)i << 4);
        for (int i = threadIdx.x; i < n_cl; i += blockDim.x) *reinterpret_cast<uint4*>(s_cls + ((uint32_t)i << 4)) = ld<uint4>(st.cls2, (uint32_t)i << 4);
    }
    GW_ROLLOUT_SRC_STAGE
    __syncthreads();
    if (e >= N) return;

    // ---- state -> registers ----
    const uint32_t RB = GEN ? (uint32_t)st.RB : 16u * NWC;
    const uint32_t o16 = e << 4, oq = e * RB;
    const uint4 ip = ld<uint4>(st.ip, o16);
    const double2 tw = ld<double2>(st.tw, o16);
    const uint4 tk = ld<uint4>(st.tk, o16);
    typename ArrSel<GEN, DM>::rw len, tb;
    typename ArrSel<GEN, DM + 1>::rw sta;
    if constexpr (GEN) {
        uint32_t* col = s_cols + (threadIdx.x & 63);
        len.p = col; tb.p = col + DM * 64; sta.p = col + 2 * DM * 64;
        for (int i = 0; i < D; ++i) len[i] = st.qb[oq + (uint32_t)i];
        for (int j = 0; j < R; ++j) sta[j] = st.qb[oq + (uint32_t)(D + j)];
    } else {
        uint4 qw[NWC];
#pragma unroll
        for (int w = 0; w < NWC; ++w) qw[w] = ld<uint4>(st.qb, oq + 16u * w);
#pragma unroll
        for (int i = 0; i < DT; ++i) len[i] = (word_of(qw[i >> 4], (i >> 2) & 3) >> ((i & 3) * 8)) & 0xffu;
#pragma unroll
        for (int j = 0; j < DT + 1; ++j) sta[j] = (word_of(qw[(DT + j) >> 4], ((DT + j) >> 2) & 3) >> (((DT + j) & 3) * 8)) & 0xffu;
    }
    double now = tw.x, wake = tw.y;
    uint32_t tau = tk.x;
    uint32_t nbp = tk.y;                                 // (changes only where an includer resets: reset_env below)
    GwBp bpc, bpp;
    bpc.t0 = ip.x; bpc.c0 = ip.y;
    bpp.t0 = ip.z; bpp.c0 = ip.w;
    const GwBp* hist = st.bph + ((size_t)e << 7);
    uint32_t rvm = tk.z;
    int32_t last_abs = (int32_t)(tk.w & 0x7fffffffu);
    uint32_t dn = tk.w >> 31;

    constexpr bool FAST = MODE >= 1, NOLIM = MODE == 2;
    const StepMathT<FAST, NOLIM> m(c);
    const double slot = c.slot, br = c.bit_rate, hd = c.hdr_dur, hdr_bits = c.hdr_bits, interval = c.counter_interval;
    const double inv_interval = c.inv_interval, tie_filter = c.tie_filter, coded_factor = c.coded_factor;
    const bool fast_ticks = FAST || c.fast_ticks != 0;
    const bool idem = c.idem_states != 0;
    const uint32_t bound = (uint32_t)c.counter_bound, base_bytes = (uint32_t)(c.mac_hdr + c.net_hdr);
    const int mh = c.mac_hdr, pv = c.payload_value;
    uint32_t live_mask = 0u;                             // any-D kernel: bit i = sender i is in a non-terminal noise state
    if constexpr (GEN) {
        for (int i = 0; i < D; ++i) live_mask |= ((s_term[i] >> sta[i]) & 1u) ? 0u : (1u << i);
    }
    typename ArrSel<GEN, DM>::ro mult, term, inv16;
    if constexpr (GEN) {
        mult.p = st.cst->mult; mult.shift16 = 0; term.p = st.cst->term; term.shift16 = 1; inv16.p = st.cst->inv16; inv16.shift16 = 0;
    } else {
#pragma unroll
        for (int i = 0; i < DT; ++i) { mult.v[i] = (uint32_t)c.mult[i]; term.v[i] = c.term[i]; inv16.v[i] = c.inv16[i]; }
    }
#pragma unroll
    for (int i = 0; i < D; ++i) tb[i] = tau;

    Tally kt = {0, 0, 0, 0, 0};
    uint32_t k_bad = 0, fl = 0;
    int k = 0;
    GW_ROLLOUT_SRC_FIRST                                        // step 0's action
#ifdef GW_ROLLOUT_SRC_RESETS
    // gw_reset for this env between step k and step k + 1, on the registers (ct_reset_sfx_kernel, ct_step_sfx.hip): counters to 0
    // from the current tick, the interpreter cleared, the clock not rewound.  That kernel takes tau as current, so the ticks
    // up to `now` are counted first, as the tail below counts them (its GW_FLAG_TIE rule included); the queues stay lazy -- a
    // reset leaves the queued packets alone and changes only the tick -> counter-value map, and tb[] still says how far each
    // length has been brought.  The ring slot written here may be read back by this lane in a later step (gw_tick_value's
    // deep path, through `hist`): both go through st.bph with plain accesses, so the compiler orders them.
    auto reset_env = [&]() {
        uint32_t kk = 0;
        while (wake <= now) { if (wake == now) fl |= GW_FLAG_TIE; wake = wake + interval; kk++; }
        tau += kk;
        GwBp* ring = st.bph + ((size_t)e << 7);
        GwBp cur; cur.t0 = bpc.t0; cur.c0 = 0u;
        if (bpc.t0 == tau) {                                    // no tick since the newest breakpoint: overwrite it
            ring[(nbp - 1u) & GW_RING_MASK] = cur;
        } else {                                                // the newest becomes the second newest
            bpp = bpc;
            cur.t0 = tau;
            ring[nbp & GW_RING_MASK] = cur;
            nbp += 1u;
        }
        bpc = cur;
        rvm = 0u; last_abs = 0; dn = 0u;                        // interpreter.reset(): receivedValues, lastAbs, done
    };
#endif
#ifdef GW_ROLLOUT_SRC_QUEUES
    // Every queue at the env's current time, for a source that chooses the action from the lengths (GW_ROLLOUT_SRC_TAKE may
    // call it): the ticks up to `now` counted as reset_env and the tail count them (GW_FLAG_TIE rule included), then every
    // length brought to that tick.  gw_len_after_ticks is additive over a split of the ticks, in the length and in both
    // tallied terms, so what the lazy form derives from them stays what it was.
    auto queues_now = [&]() {
        uint32_t kk = 0;
        while (wake <= now) { if (wake == now) fl |= GW_FLAG_TIE; wake = wake + interval; kk++; }
        tau += kk;
#pragma unroll
        for (int i = 0; i < D; ++i) { len[i] = gw_len_after_ticks(len[i], tau - tb[i], mult[i], kt); tb[i] = tau; }
    };
#endif
    auto put_feedback = [&](int32_t latest, int32_t r) {
        const size_t at = (size_t)k * N + e;
        GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)
        k++;
    };

    while (k < K) {
        // ---- start of step k (counter_traffic.py:146-158) ----
        GW_ROLLOUT_SRC_TAKE
        if (GW_ROLLOUT_SRC_CHECKED((unsigned)d >= (unsigned)D || (unsigned)du >= (unsigned)c.max_duration)) {
            fl |= GW_FLAG_BADACT;                    // env untouched, feedback repeats the current values
            k_bad++;
            put_feedback(pv * ((int)(rvm & 1u) - (int)((rvm >> 1) & 1u)), 0);
            continue;
        }
        uint32_t l0 = 0, t0 = 0, s_d_old = 0, mult_d = 0, inv16_d = 65536u;
        if constexpr (GEN) {
            l0 = len[d]; t0 = tb[d]; s_d_old = sta[d];
            mult_d = s_mi[d].x; inv16_d = s_mi[d].y;
        } else {
#pragma unroll
            for (int i = 0; i < D; ++i)
                if (i == d) { l0 = len[i]; t0 = tb[i]; mult_d = mult[i]; inv16_d = inv16[i]; s_d_old = sta[i]; }
        }
        uint32_t len_d = gw_len_after_ticks(l0, tau - t0, mult_d, kt);          // the addressed queue, up to date
        const int slots = du * c.duration_factor;                               // counter_traffic.py:149
        const int Ld = ndigits(slots);
        const bool cls_valid = NOLIM || now < c.cls_limit;
        const uint32_t s_d = s_trans[(uint32_t)((d * R + RRM) * S) + s_d_old];  // d after hearing the RRM
#pragma unroll
        for (int i = 0; i < (GEN ? 0 : D); ++i) if (i == d) sta[i] = s_d;
        if constexpr (GEN) {
            sta[d] = s_d;
            live_mask = ((s_term[d] >> s_d) & 1u) ? (live_mask & ~(1u << d)) : (live_mask | (1u << d));
        }
        // ---- A.1 / A.2: announcement ----
        const TxTimes an = tx_times(m, now, hd, m.over_rate((double)(Ld * 8)));
        kt.tx++;
        const bool granted = decode(m, (uint32_t)s_cls[(uint32_t)(d * S) + s_d], cls_valid, s_ber[(uint32_t)(d * S) + s_d], an, br, hdr_bits,
                                    (double)(Ld * 8) * coded_factor, fl);
        const double t_r = an.t_e;
        const double t_end = t_r + (double)(slots + 1) * slot;                  // simple_stack.py:557-558
        uint32_t s_r = sta[RRM];
        uint32_t n_data = 0;

        // counter ticks with wake < t (or <= t): the running sum four at a time, or one jump where the step qualifies
        auto ticks_to = [&](double t, bool inclusive) {
            uint32_t kk = 0;
            for (;;) {
                const double w1 = wake + interval, w2 = w1 + interval, w3 = w2 + interval, w4 = w3 + interval;
                const bool b0 = inclusive ? (wake <= t) : (wake < t);
                const bool b1 = inclusive ? (w1 <= t) : (w1 < t);
                const bool b2 = inclusive ? (w2 <= t) : (w2 < t);
                const bool b3 = inclusive ? (w3 <= t) : (w3 < t);
                const double last = b3 ? w3 : (b2 ? w2 : (b1 ? w1 : wake));
                if (inclusive && b0 && last == t) fl |= GW_FLAG_TIE;
                kk += (uint32_t)b0 + (uint32_t)b1 + (uint32_t)b2 + (uint32_t)b3;
                wake = b3 ? w4 : (b2 ? w3 : (b1 ? w2 : (b0 ? w1 : wake)));
                if (!b3) break;
            }
            tau += kk;
            len_d = gw_len_after_ticks(len_d, kk, mult_d, kt);
        };
        double delta = 0.0;
        const bool span_ok = fast_ticks && gw_tick_span_ok(wake, t_end, interval, &delta);
        auto ticks_upto = [&](double t, bool inclusive) {
            uint32_t nj = 0;
            double wj = wake;
            bool tiej = false, sane = false;
            gw_tick_jump_lo(wake, t, delta, c.inv_interval_lo, inclusive, &nj, &wj, &tiej, &sane);
            if (span_ok && sane) {
                wake = wj;
                tau += nj;
                if (tiej) fl |= GW_FLAG_TIE;
                len_d = gw_len_after_ticks(len_d, nj, mult_d, kt);
            } else {
                ticks_to(t, inclusive);
            }
        };

        if (granted) {
            // ---- A.3 / A.4: window at sender d (simple_stack.py:397-434) ----
            const double stopw = t_r + (double)slots * slot;                    // :400-401
            double cur = t_r;
            ticks_upto(cur, false);                   // (covers the ticks since the previous window closed too: counting is cumulative)
            const uint32_t s_r1 = s_trans[(uint32_t)((RRM * R + d) * S) + s_r];            // the RRM after one packet of d
            const double ber_x1 = s_ber[(uint32_t)((D + d) * S) + s_r1];
            const uint32_t cls_x1 = s_cls[(uint32_t)((D + d) * S) + s_r1];
            bool more = true;
            uint32_t pops = 0;
            {
                // the straight-line form: preconditions and reasoning in ct_step_sfx.hip
                const double span = t_end - t_r;
                const bool straight = span_ok && mult_d != 0u && idem && cls_valid && cls_x1 != (uint32_t)GW_CLS_COMPUTE &&
                                      (FAST || (m.fast_fmod && m.fast_div)) && (NOLIM || t_end < m.fmod_limit) && t_r >= span + span;
                if (straight && len_d != 0u) {
                    auto head = [&](uint32_t ln, uint32_t tk_now, bool& deep) {
                        const uint32_t age = __umul24(ln + mult_d - 1u, inv16_d) >> 16;   // gw_ceil_div
                        const uint32_t ht = tk_now - age;
                        const bool older = ht < bpc.t0;
                        deep = older && ht < bpp.t0;
                        return base_bytes + gw_min_u32((older ? bpp.c0 : bpc.c0) + (ht - (older ? bpp.t0 : bpc.t0)), bound);
                    };
                    bool deep = false;
                    uint32_t chk = 0;
                    uint32_t sz = head(len_d, tau, deep);
                    bool go = !deep && (stopw - cur) > gw_fast_div((double)(sz * 8u), m.dr, m.rcp_dr);
                    while (go) {
                        const double pd = gw_fast_div((double)(((int)sz - mh) * 8), m.dr, m.rcp_dr);
                        const double t_s = cur + (m.slot - gw_fast_fmod_lo(cur, m.slot, c.inv_slot_lo));
                        const double t_e = t_s + (hd + pd);
                        uint32_t nj = 0;
                        double wj = wake;
                        bool tiej = false, sane = false;
                        gw_tick_jump_lo(wake, t_e, delta, c.inv_interval_lo, true, &nj, &wj, &tiej, &sane);
                        chk |= (sane ? 0u : (uint32_t)GW_FLAG_INTERNAL) | (tiej ? (uint32_t)GW_FLAG_TIE : 0u);
                        len_d = gw_min_u32(len_d - 1u + __umul24(nj, mult_d), (uint32_t)GW_QUEUE_CAP);
                        tau += nj;
                        wake = wj;
                        cur = t_e;
                        pops++;
                        bool deep_n = false;
                        sz = head(len_d, tau, deep_n);
                        go = cur < stopw && len_d != 0u && !deep_n && (stopw - cur) > gw_fast_div((double)(sz * 8u), m.dr, m.rcp_dr);
                    }
                    (void)head(len_d, tau, deep);
                    more = cur < stopw && (len_d == 0u || deep);
                    fl |= chk | ((pops && !(cur < t_end)) ? (uint32_t)GW_FLAG_CARRY : 0u);
                }
            }
            if (pops) {                                                         // devices.py:163-168, counter_traffic.py:75-80
                const bool okx = cls_x1 == (uint32_t)GW_CLS_OK;
                kt.pop += pops;
                kt.tx += pops;
                n_data += pops;
                s_r = s_r1;
                kt.deliv += okx ? pops : 0u;
                rvm |= okx ? (1u << d) : 0u;
                dn = (okx && pv == c.counter_bound) ? 1u : dn;
            }
            if (more)
            for (;;) {
                if (len_d == 0u) {                                              // :409-416
                    if (mult_d != 0u && wake < stopw) {
                        cur = wake;
                        wake = wake + interval;
                        tau++;
                        len_d = gw_len_after_ticks(0u, 1u, mult_d, kt);
                    } else break;
                }
                const uint32_t age = gw_ceil_div(len_d, mult_d, inv16_d);
                const uint32_t sz = base_bytes + gw_tick_value(tau - age, bpc, bpp, nbp, hist, bound);
                const double need = m.over_rate((double)(sz * 8u));             // messages.py:67-75
                if (!((stopw - cur) > need)) break;                             // :418-420
                len_d--;                                                        // :425
                kt.pop++;
                const int pay = (int)sz - mh;
                const TxTimes x = tx_times(m, cur, hd, m.over_rate((double)(pay * 8)));
                kt.tx++;
                n_data++;
                s_r = s_trans[(uint32_t)((RRM * R + d) * S) + s_r];             // the RRM hears sender d (again)
                const bool ok = decode(m, (uint32_t)s_cls[(uint32_t)((D + d) * S) + s_r], cls_valid, s_ber[(uint32_t)((D + d) * S) + s_r], x, br,
                                       hdr_bits, (double)(pay * 8) * coded_factor, fl);
                kt.deliv += ok ? 1u : 0u;
                rvm |= ok ? (1u << d) : 0u;
                dn = (ok && pv == c.counter_bound) ? 1u : dn;
                fl |= !(x.t_e < t_end) ? (uint32_t)GW_FLAG_CARRY : 0u;
                ticks_upto(x.t_e, true);                                        // ticks are older events than the MAC's resume
                cur = x.t_e;
                if (!(cur < stopw)) break;                                      // window timeout already processed
            }
        }

        // ---- close the step: A.5 lazily (the ticks up to t_end are counted by the next step's first count); what must not be
        //      lost is the diagnostic bit for a tick falling EXACTLY on t_end (see the event loop above) ----
        {
            const double dd = t_end - wake;
            if (dd >= 0.0) {
                const double q = dd * inv_interval;
                if (!(fabs(q - rint(q)) > tie_filter) || !(wake >= 0.0625) || !(wake < 2097152.0)) {
                    for (double w = wake; w <= t_end; w = w + interval)
                        if (w == t_end) fl |= GW_FLAG_TIE;
                }
            }
        }
        bool all_term = true;
        if constexpr (GEN) {
            all_term = (live_mask & ~(1u << d)) == 0u;
            len[d] = len_d; tb[d] = tau;
        } else {
#pragma unroll
            for (int i = 0; i < D; ++i) all_term = all_term && (i == d || ((term[i] >> sta[i]) & 1u));
#pragma unroll
            for (int i = 0; i < D; ++i)
                if (i == d) { len[i] = len_d; tb[i] = tau; }
        }
        if (!all_term) {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                if (i == d) continue;
                uint32_t si = s_trans[(uint32_t)((i * R + RRM) * S) + sta[i]];  // heard the announcement
                for (uint32_t n = 0; n < n_data; ++n) {                          // ... and d's data
                    const uint32_t s2 = s_trans[(uint32_t)((i * R + d) * S) + si];
                    if (s2 == si) break;
                    si = s2;
                }
                sta[i] = si;
                if constexpr (GEN) live_mask = ((term[i] >> si) & 1u) ? (live_mask & ~(1u << i)) : (live_mask | (1u << i));
            }
        }
        sta[RRM] = s_r;
        const int32_t latest = pv * ((int)(rvm & 1u) - (int)((rvm >> 1) & 1u));
        const int32_t abs_d = latest < 0 ? -latest : latest;
        int32_t r = last_abs - abs_d;
        last_abs = abs_d;
        r = r > 10 ? 10 : (r < -10 ? -10 : r);
        now = t_end;
        put_feedback(latest, r);
    }

    // ---- catch up: ticks up to the end of the last step, every queue to the final tick ----
    {
        uint32_t kk = 0;
        while (wake <= now) { if (wake == now) fl |= GW_FLAG_TIE; wake = wake + interval; kk++; }
        tau += kk;
#pragma unroll
        for (int i = 0; i < D; ++i) len[i] = gw_len_after_ticks(len[i], tau - tb[i], mult[i], kt);
    }
    if constexpr (GEN) {
        for (int i = 0; i < D; ++i) st.qb[oq + (uint32_t)i] = (uint8_t)len[i];
        for (int j = 0; j < R; ++j) st.qb[oq + (uint32_t)(D + j)] = (uint8_t)sta[j];
    } else {
        uint32_t nb[16 * NWC];
#pragma unroll
        for (int b = 0; b < 16 * NWC; ++b) nb[b] = 0u;
#pragma unroll
        for (int i = 0; i < DT; ++i) nb[i] = len[i];
#pragma unroll
        for (int j = 0; j < DT + 1; ++j) nb[DT + j] = sta[j];
#pragma unroll
        for (int w = 0; w < NWC; ++w) {
            const int b = 16 * w;
            uint4 o;
            o.x = nb[b + 0] | (nb[b + 1] << 8) | (nb[b + 2] << 16) | (nb[b + 3] << 24);
            o.y = nb[b + 4] | (nb[b + 5] << 8) | (nb[b + 6] << 16) | (nb[b + 7] << 24);
            o.z = nb[b + 8] | (nb[b + 9] << 8) | (nb[b + 10] << 16) | (nb[b + 11] << 24);
            o.w = nb[b + 12] | (nb[b + 13] << 8) | (nb[b + 14] << 16) | (nb[b + 15] << 24);
            st_plain(st.qb, oq + 16u * w, o);
        }
    }
    st_plain(st.tw, o16, make_double2(now, wake));
    st_plain(st.tk, o16, make_uint4(tau, nbp, rvm, (uint32_t)last_abs | (dn << 31)));
    publish_env_counters(st.sa, N, e, kt.pop, kt.deliv, k_bad, fl, (uint32_t)K);
#undef GW_ROLLOUT_SRC_RESETS
#undef GW_ROLLOUT_SRC_QUEUES
#undef GW_ROLLOUT_SRC_STAGE
#undef GW_ROLLOUT_SRC_FIRST
#undef GW_ROLLOUT_SRC_TAKE
#undef GW_ROLLOUT_SRC_CHECKED
#undef GW_ROLLOUT_SRC_STEPPED
