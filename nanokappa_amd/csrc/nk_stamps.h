// nk_stamps.h -- developer build NK_STAMPS (make stamps): the report of the clock stamps the sweep, k_emit and k_events leave in
// NkDev::stamps, printed after every batch.  Host code only; included by nk_engine.hip below nk_ctx and NK_HIP, which it uses.
#pragma once

// "[stamps] <what>: min .. [p10 ..] median .. mean .. p<hi> .. max .." of v with `prec` decimals; hi = 90 or 99
static void nk_stamps_quantiles(std::vector<double> v, const std::string &what, int prec, bool p10, int hi) {
    if (v.empty()) return;
    std::sort(v.begin(), v.end());
    double sm = 0; for (double x : v) sm += x;
    const size_t n = v.size();
    fprintf(stderr, "[stamps] %s: min %.*f", what.c_str(), prec, v.front());
    if (p10) fprintf(stderr, "  p10 %.*f", prec, v[n / 10]);
    fprintf(stderr, "  median %.*f  mean %.*f  p%d %.*f  max %.*f\n", prec, v[n / 2], prec, sm / n, hi, prec,
            v[hi == 99 ? (size_t)(n * 0.99) : n * 9 / 10], prec, v.back());
}

// section shares of the LAST sweep of the batch
static int nk_stamps_report(nk_ctx *ctx) {
    const NkDev &d = ctx->d;
    if (!d.stamps) return NK_OK;
    std::vector<unsigned long long> st((size_t)d.nseg * 16);
    NK_HIP(hipMemcpy(st.data(), d.stamps, st.size() * 8, hipMemcpyDeviceToHost));
    double sum[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int sgm = 0; sgm < d.nseg; ++sgm) for (int k = 0; k < 7; ++k) sum[k] += (double)st[(size_t)sgm * 8 + k];
    double tot = 0; for (int k = 0; k < 6; ++k) tot += sum[k];
    {   // in-kernel shader clock of the sweep (s_memtime against the 100 MHz s_memrealtime, per segment; median)
        std::vector<unsigned long long> clk;
        for (int sgm = 0; sgm < d.nseg; ++sgm) clk.push_back(st[(size_t)sgm * 8 + 7]);
        std::sort(clk.begin(), clk.end());
        // wall-clock marks (10 ns ticks of the 100 MHz counter): where the launch's time goes outside the tile loops
        unsigned long long e0 = ~0ull, x1 = 0;
        std::vector<double> pro, loop, epi, fin;
        for (int sgm = 0; sgm < d.nseg; ++sgm) {
            const unsigned long long *w = &st[((size_t)d.nseg + sgm) * 8];
            if (!w[0] || !w[3]) continue;
            e0 = std::min(e0, w[0]); x1 = std::max(x1, w[3]);
        }
        for (int sgm = 0; sgm < d.nseg; ++sgm) {
            const unsigned long long *w = &st[((size_t)d.nseg + sgm) * 8];
            if (!w[0] || !w[3]) continue;
            pro.push_back((double)(w[1] - w[0]) * 0.01); loop.push_back((double)(w[2] - w[1]) * 0.01);
            epi.push_back((double)(w[3] - w[2]) * 0.01); fin.push_back((double)(w[3] - e0) * 0.01);
        }
        auto q = [](const std::vector<double> &v, const char *nm) { nk_stamps_quantiles(v, std::string(nm) + " [us]", 1, true, 90); };
        {   // k_emit's marks of the same step (words 4-7 of the second row): entry, tables in LDS, first entries evaluated, done
            unsigned long long m0 = ~0ull, m3 = 0;
            std::vector<double> a, b, c, fin2;
            for (int sgm = 0; sgm < d.nseg; ++sgm) { const unsigned long long *w = &st[((size_t)d.nseg + sgm) * 8 + 4]; if (w[0] && w[3]) { m0 = std::min(m0, w[0]); m3 = std::max(m3, w[3]); } }
            for (int sgm = 0; sgm < d.nseg; ++sgm) {
                const unsigned long long *w = &st[((size_t)d.nseg + sgm) * 8 + 4];
                if (!w[0] || !w[3]) continue;
                a.push_back((double)(w[1] - w[0]) * 0.01); b.push_back((double)(w[2] - w[1]) * 0.01); c.push_back((double)(w[3] - w[2]) * 0.01);
                fin2.push_back((double)(w[3] - m0) * 0.01);
            }
            auto q2 = [](const std::vector<double> &v, const char *nm) { nk_stamps_quantiles(v, std::string("k_emit ") + nm + " [us]", 1, false, 90); };
            if (!a.empty()) {
                fprintf(stderr, "[stamps] k_emit first entry -> last wave done: %.1f us\n", (double)(m3 - m0) * 0.01);
                q2(a, "entry -> tables in LDS"); q2(b, "-> first chunk of entries evaluated"); q2(c, "-> particles built and stored"); q2(fin2, "wave done, after the first entry");
            }
        }
        fprintf(stderr, "[stamps] first entry -> last exit: %.1f us over %zu waves\n", (double)(x1 - e0) * 0.01, pro.size());
        {   // where do the slow waves sit?  mean tile-loop time by workgroup index mod 8 (the XCD under round-robin placement),
            // by wave within the workgroup, and by thirds of the grid
            double xs[8] = {0}, xn[8] = {0}, ws[4] = {0}, wn[4] = {0}, gs[4] = {0}, gn[4] = {0}, rs[8] = {0}, rn[8] = {0};
            for (int sgm = 0; sgm < d.nseg; ++sgm) {
                const unsigned long long *w = &st[((size_t)d.nseg + sgm) * 8];
                if (!w[0] || !w[3]) continue;
                const double t = (double)(w[2] - w[1]) * 0.01;
                const int wg = sgm / 4;
                xs[wg % 8] += t; xn[wg % 8] += 1; ws[sgm % 4] += t; wn[sgm % 4] += 1;
                const int third = (int)((int64_t)sgm * 4 / d.nseg); gs[third] += t; gn[third] += 1;
                const int rk = wg / ctx->num_cu; if (rk < 8) { rs[rk] += t; rn[rk] += 1; }
            }
            fprintf(stderr, "[stamps] tile loop mean [us] by workgroup %% 8:");
            for (int k = 0; k < 8; ++k) fprintf(stderr, " %.1f", xn[k] ? xs[k] / xn[k] : 0.0);
            fprintf(stderr, " | by wave of the workgroup:");
            for (int k = 0; k < 4; ++k) fprintf(stderr, " %.1f", wn[k] ? ws[k] / wn[k] : 0.0);
            fprintf(stderr, " | by quarter of the grid:");
            for (int k = 0; k < 4; ++k) fprintf(stderr, " %.1f", gn[k] ? gs[k] / gn[k] : 0.0);
            fprintf(stderr, " | by workgroup / CUs (the k-th workgroup of a CU under in-order dispatch):");
            for (int k = 0; k < 8; ++k) if (rn[k]) fprintf(stderr, " %.1f", rs[k] / rn[k]);
            fprintf(stderr, "\n");
        }
        q(pro, "entry -> tile loop (tables into LDS, records)"); q(loop, "tile loop"); q(epi, "tile loop end -> wave through (flush, workgroup barrier, tally row)");
        q(fin, "wave through, after the first entry");
        fprintf(stderr, "[stamps] shader clock inside k_sweep: median %.0f MHz (min %.0f, max %.0f)\n", clk[clk.size() / 2] / 10.0, clk.front() / 10.0, clk.back() / 10.0);
    }
    fprintf(stderr, "[stamps] cycles per tile: arrive %.0f  relax+drift %.0f  tally+store %.0f  pack/merge %.0f  event %.0f  event tally/store/repack %.0f  | total %.0f (tiles %.0f)\n",
            sum[0] / sum[6], sum[1] / sum[6], sum[2] / sum[6], sum[3] / sum[6], sum[4] / sum[6], sum[5] / sum[6], tot / sum[6], sum[6]);
    if (d.qx) {                                     // split sweep: k_events' per-segment clocks (words 3-5)
        std::vector<double> cyc, wk, qq, ps;
        for (int sgm = 0; sgm < d.nseg; ++sgm) {
            cyc.push_back((double)st[(size_t)sgm * 8 + 3]); wk.push_back((double)st[(size_t)sgm * 8 + 4]);
            qq.push_back((double)(st[(size_t)sgm * 8 + 5] >> 32)); ps.push_back((double)(st[(size_t)sgm * 8 + 5] & 0xffffffffull));
        }
        auto stat = [](const std::vector<double> &v, const char *nm) { nk_stamps_quantiles(v, std::string("k_events per segment ") + nm, 0, false, 99); };
        stat(cyc, "cycles"); stat(wk, "cycles in walks"); stat(qq, "queue entries"); stat(ps, "walk passes");
        std::vector<double> lc, ln;
        for (int sgm = 0; sgm < d.nseg; ++sgm) { lc.push_back((double)(st[(size_t)sgm * 8 + 6] & ((1ull << 40) - 1))); ln.push_back((double)(st[(size_t)sgm * 8 + 6] >> 40)); }
        stat(lc, "cycles in faces passes"); stat(ln, "faces passes");
    }
    return NK_OK;
}
