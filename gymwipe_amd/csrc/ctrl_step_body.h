// ctrl_step_body.h -- one env.step() of the closed control loop for one lane: the body of ctrl_step_kernel (ctrl_step.hip, where
// the rules and their sources are stated), moved here word for word so that the fused kernels of ctrl_rollout.hip run the same
// step.  Text included inside a kernel, not a function, as ct_rollout_sync_body.h is and for its reason: as a __forceinline__
// function ctrl_step_kernel came out with other registers (accum_offset 164 -> 168); included, it is instruction for instruction
// what it was.
// The including kernel provides, in scope: c (GwCtrlDev), k (GwDevConst), S (= GW_MAX_NSTATES), s_trans / s_ber (the link tables
// in LDS, [CR][CR][S]), L (Lane), q0 / q1 (Q, opened: q_open), col0 / col1 (the lane's LDS columns), ring0 / ring1 (its rings),
// deg_per_rad, and the step's action `const int d, du`.  The text defines no name outside its own braces.
// The controller's rule is a compile-time switch, a preprocessor symbol because the text is no template: included with
// GW_CTRL_PID defined, the controller is the reference's three-term PID on the env's own gains and last error, G (Pid), which the
// including kernel then provides as well; included without, it is the same rule at gains (1, 0, 0), folded, and no G is named.
// The plant disturbance is a second switch, GW_CTRL_DIST, only ever defined together with GW_CTRL_PID: every substep then ends
// with one draw of the env's own counter-based noise added to the plant's state (gw_ctrl_set_disturbance in
// include/gymwipe_amd.h), on W (Dist), which the including kernel provides; without it no W is named and the plant is exact.
    if ((unsigned)d >= 2u || (unsigned)du >= (unsigned)k.max_duration) {
        L.fl |= GW_FLAG_BADACT;                              // envs/inverted_pendulum.py:102 asserts; flagged and skipped here
    } else {
        const StepMath m(k);
        const double slot = k.slot, br = k.bit_rate, hd = k.hdr_dur, hdr_bits = k.hdr_bits, interval = k.counter_interval;
        const int mh = k.mac_hdr;
#ifdef GW_CTRL_LOSS
        // the step's two links, selected once: the announcement's (0 or 1) and the data packets' (2 or 3); X is never indexed by d
        const uint32_t thr_an = d == 0 ? X.thr[0] : X.thr[1], thr_da = d == 0 ? X.thr[2] : X.thr[3];
        uint32_t lost_an = 0u, lost_da = 0u;
#endif
        double* ringd = d == 0 ? ring0 : ring1;
        // the first PRE values at the head of the addressed queue, issued now: they land during the announcement
        double pre[PRE];
        {
            const uint32_t h0 = d == 0 ? q0.head : q1.head;
#pragma unroll
            for (int i = 0; i < PRE; ++i) pre[i] = ringd[(h0 + (uint32_t)i) & GW_RING_MASK];
        }
        // the control tick test `(tick - start) % period == 0` as a running phase: one modulo per step, not per tick
        uint32_t phase = L.ktick >= c.start ? (L.ktick - c.start) % c.period : 0u;

        // one counter tick: the sensor's process was created first, so it runs first at every tick time
        auto tick_all = [&]() __attribute__((always_inline)) {
            q_push(q0, col0, L.x[2]);                                           // sensor: sample, queue, ...
            double nx[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {                                      // ... then the plant advances one substep
                double acc = c.A[i * 4 + 0] * L.x[0];
                acc = acc + c.A[i * 4 + 1] * L.x[1];
                acc = acc + c.A[i * 4 + 2] * L.x[2];
                acc = acc + c.A[i * 4 + 3] * L.x[3];
                nx[i] = acc + c.B[i] * L.u;
            }
#ifdef GW_CTRL_DIST
            {                                                                  // ... and is pushed: x = nx + g * w, the product
                const double w = dist_draw(W);                                 // rounded, then the sum (no contraction); n += 1
#pragma unroll
                for (int i = 0; i < 4; ++i) L.x[i] = nx[i] + W.g[i] * w;
            }
#else
#pragma unroll
            for (int i = 0; i < 4; ++i) L.x[i] = nx[i];
#endif
            L.nsub++;
            const uint32_t kk = L.ktick;                                        // controller
            if (kk >= c.start) {
#ifdef GW_CTRL_PID
                if (phase == 0u) {                                              // control(), control/inverted_pendulum.py:54-68:
                    const double err = fabs(L.ang);                             // abs(sp - angle), sp = 0
                    const double pid = ((G.kp * err) + (G.ki * (err + G.last))) + (G.kd * (err - G.last));
                    G.last = err;                                               // calcVelocity runs whether or not anything is sent
                    if (L.ang != 0.0) {
                        q_push(q1, col1, L.ang < 0.0 ? pid : -pid);
                        L.ncmd++;
                    }
                }
#else
                if (phase == 0u && L.ang != 0.0) {                              // the same rule at gains (1, 0, 0)
                    q_push(q1, col1, -L.ang);
                    L.ncmd++;
                }
#endif
                phase = phase + 1u == c.period ? 0u : phase + 1u;
            }
            L.ktick = kk + 1u;
            L.wake = L.wake + interval;                                         // running sum, as everywhere
        };
        auto ticks_until = [&](double t, bool inclusive) __attribute__((always_inline)) {
            while (inclusive ? (L.wake <= t) : (L.wake < t)) {
                if (L.wake == t) L.fl |= GW_FLAG_TIE;
                tick_all();
            }
        };
        // every radio but `from` hears a transmission: its noise state moves (simple_stack.py:130-157)
        auto all_hear = [&](int from) {
#pragma unroll
            for (int j = 0; j < CR; ++j)
                if (j != from) L.rxs[j] = s_trans[(j * CR + from) * S + L.rxs[j]];  // j is a compile-time index here
        };

        const double t_a = L.now;
        const int slots = du * k.duration_factor;
        const int Ld = ndigits(slots);
        const TxTimes an = tx_times(m, t_a, hd, m.over_rate((double)(Ld * 8)));
        L.ntx++;
        all_hear(CRRM);
#ifdef GW_CTRL_LOSS
        const bool heard = receive(m, s_ber[(d * CR + CRRM) * S + pick(L.rxs, d)], an, br, hdr_bits,
                                   (double)(Ld * 8) * k.coded_factor, L.fl);
        const bool erased_an = loss_draw(X, thr_an);                            // drawn whatever the PHY decided: no short circuit
        lost_an += erased_an ? 1u : 0u;
        const bool granted = heard & !erased_an;                                // an erased announcement is an ungranted step
#else
        const bool granted = receive(m, s_ber[(d * CR + CRRM) * S + pick(L.rxs, d)], an, br, hdr_bits,
                                     (double)(Ld * 8) * k.coded_factor, L.fl);
#endif
        const double t_r = an.t_e;
        const double t_end = t_r + (double)(slots + 1) * slot;
        if (granted) {
            const double stopw = t_r + (double)slots * slot;
            double cur = t_r;
            ticks_until(cur, false);                                            // the MAC's initialisation is URGENT: it goes first
            const int dst = d + 1;                                              // sensor -> controller, controller -> actuator
            const uint32_t sz = (uint32_t)(k.mac_hdr + k.net_hdr) + (d == 0 ? 2u : 1u);
            const double need = m.over_rate((double)(sz * 8u));
            const double pd = m.over_rate((double)(((int)sz - mh) * 8));
            for (;;) {
                bool closed = false;
                while ((d == 0 ? q0.len : q1.len) == 0u) {                      // wait for packet-added or the window timeout
                    if (L.wake < stopw) { cur = L.wake; tick_all(); }
                    else { closed = true; break; }
                }
                if (closed) break;
                if (!((stopw - cur) > need)) break;
                // the head value (a tick may have dropped older entries meanwhile: head/len say where the head is now)
                Q& qd = d == 0 ? q0 : q1;
                double v;
                if (qd.len <= qd.app) {                                         // appended in this step: from the LDS column
                    v = (d == 0 ? col0 : col1)[(qd.app - qd.len) << 6];
                } else {
                    const uint32_t i = (qd.head - qd.head0) & GW_RING_MASK;     // how many older entries have gone already
                    if (i < (uint32_t)PRE) {
                        v = pre[0];
#pragma unroll
                        for (int j = 1; j < PRE; ++j) v = (i == (uint32_t)j) ? pre[j] : v;
                    } else {
                        v = ringd[qd.head];
                    }
                }
                qd.head = (qd.head + 1u) & GW_RING_MASK;
                qd.len--;
                const TxTimes x = tx_times(m, cur, hd, pd);
                L.ntx++;
                all_hear(d);
#ifdef GW_CTRL_LOSS
                const bool decoded = receive(m, s_ber[(dst * CR + d) * S + pick(L.rxs, dst)], x, br, hdr_bits,
                                             (double)(((int)sz - mh) * 8) * k.coded_factor, L.fl);
                const bool erased = loss_draw(X, thr_da);                       // popped, sent and heard by every radio; not delivered
                lost_da += erased ? 1u : 0u;
                const bool ok = decoded & !erased;
#else
                const bool ok = receive(m, s_ber[(dst * CR + d) * S + pick(L.rxs, dst)], x, br, hdr_bits,
                                        (double)(((int)sz - mh) * 8) * k.coded_factor, L.fl);
#endif
                if (!(x.t_e < t_end)) L.fl |= GW_FLAG_CARRY;
                ticks_until(x.t_e, true);                                       // ticks during the transmission, one exactly on its end
                if (ok) {                                                       // included; then the delivery at t_e
                    if (d == 0) { L.ang = v * deg_per_rad; L.got1++; }          // degrees(value), control/inverted_pendulum.py:41
                    else { L.u = v; L.got2++; }
                }
                cur = x.t_e;
                if (!(cur < stopw)) break;
            }
        }
        ticks_until(t_end, true);
        L.now = t_end;
#ifdef GW_CTRL_LOSS
        X.lost[0] += d == 0 ? lost_an : 0u; X.lost[1] += d == 0 ? 0u : lost_an;
        X.lost[2] += d == 0 ? lost_da : 0u; X.lost[3] += d == 0 ? 0u : lost_da;
#endif
    }
