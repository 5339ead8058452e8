// The body of plan_mppi_kernel and plan_mppi_uni_kernel (plan_kernels.h), #included into each: the ranks, the best row, the
// softmax weights and the weighted mean / deviation; the clip of the action alone depends on the robot.  In scope: UNI (constexpr
// bool), max_rotation (0.0 without UNI) and the kernel's arguments.
    __shared__ double sc[kPlanMaxCandidates];
    __shared__ double wt[kPlanMaxCandidates];
    __shared__ double first[2];
    __shared__ int top_k;
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    const double held = best_score[b];  // (read by every lane before lane 0 may replace it below)
    for (int k = lane; k < K; k += 64) sc[k] = score[b * K + k];
    if (lane == 0) top_k = 0;  // (NaN scores rank nothing sensibly; the index read below still addresses the env's own candidates)
    __syncthreads();
    for (int k = lane; k < K; k += 64) {
        const int rank = plan_rank(sc, K, k);
        if (order) order[b * K + rank] = k;
        if (rank == 0) top_k = k;
    }
    __syncthreads();
    const int top = top_k;
    const double s_top = sc[top];
    if (!keep_best || s_top > held) {  // strict: the earliest holder of a score keeps it
        const double2* src = candidates + (b * K + top) * n;
        for (int t = lane; t < n; t += 64) best_actions[b * n + t] = src[t];
        if (lane == 0) best_score[b] = s_top;
    }
    for (int k = lane; k < K; k += 64) wt[k] = exp((sc[k] - s_top) / temperature);
    __syncthreads();
    double Z = 0.0;
    for (int k = 0; k < K; ++k) Z = Z + wt[k];
    const double* cand = reinterpret_cast<const double*>(candidates) + b * K * n * 2;
    const double keep = 1.0 - smoothing;
    for (int c = lane; c < 2 * n; c += 64) {  // component (t, xy) of the plan: sums over all candidates in index order
        double num = 0.0;
        for (int k = 0; k < K; ++k) num = num + wt[k] * cand[(size_t)k * n * 2 + c];
        const double m = num / Z;
        const size_t at = b * n * 2 + c;
        const double updated = smoothing * mean[at] + keep * m;
        mean[at] = updated;
        if (c < 2) first[c] = updated;
        if (fit_std) {
            double dev2 = 0.0;
            for (int k = 0; k < K; ++k) {
                const double d = cand[(size_t)k * n * 2 + c] - m;
                dev2 = dev2 + wt[k] * (d * d);
            }
            const double sd = sqrt(dev2 / Z);
            const double blended = smoothing * std[at] + keep * sd;
            std[at] = blended < min_std ? min_std : blended;
        }
    }
    __syncthreads();
    if (lane == 0) {
        double2 a = make_double2(first[0], first[1]);
        if (UNI) {
            a = plan_clip_uni(a, rv[b * A].y, max_rotation);
        } else {
            const double nrm = sqrt(a.x * a.x + a.y * a.y), v_pref = rv[b * A].y;
            if (nrm > v_pref) {
                const double s = v_pref / nrm;
                a.x *= s, a.y *= s;
            }
        }
        action[b] = a;
    }
