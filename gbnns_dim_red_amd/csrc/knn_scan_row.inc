// knn_scan_row.inc -- statements, not a header: the distances of ONE staged base row to the QPT queries a thread holds in registers, in the
// reference's own arithmetic.  Included inside the row loop of knn_scan_kernel (knn.hip) and knn_gather_kernel (knn_gather.hip), where
//   METRIC, S, QPT   the kernel's template arguments (S = 16-byte steps of a query in registers, d <= 4 * S; QPT = queries per thread)
//   trow             const float4*: the row's S steps in LDS (zero from the row's last whole step on), the same address in every lane
//   q                float4 [QPT][S]: the thread's queries
//   dist             float [QPT]: written here
// are in scope.  f32x2: knn_scan_dist.h.
    if constexpr (METRIC == 0) {
        // two-wide vectors so that the compiler emits v_pk_add_f32 / v_pk_mul_f32 (each lane of a packed
        // instruction is an ordinary IEEE operation: same results as the scalar form)
        f32x2 s01[QPT], s23[QPT];
#pragma unroll
        for (int a = 0; a < QPT; ++a) s01[a] = s23[a] = f32x2{0.f, 0.f};
#pragma unroll
        for (int c = 0; c < S; ++c) {
            const float4 b = trow[c];  // same address in every lane: LDS broadcast
            const f32x2 b01{b.x, b.y}, b23{b.z, b.w};
#pragma unroll
            for (int a = 0; a < QPT; ++a) {  // support_func.h:113-124: e = a - b; sum += e * e, four lanes
                const f32x2 e01 = b01 - f32x2{q[a][c].x, q[a][c].y};
                const f32x2 e23 = b23 - f32x2{q[a][c].z, q[a][c].w};
                s01[a] = s01[a] + e01 * e01;
                s23[a] = s23[a] + e23 * e23;
            }
        }
#pragma unroll
        for (int a = 0; a < QPT; ++a) dist[a] = ((s01[a].x + s01[a].y) + s23[a].x) + s23[a].y;  // :125-126
    } else {
        f32x2 cs[QPT][4];  // eight running sums (k mod 8) as four pairs: {0,1} {2,3} {4,5} {6,7}
#pragma unroll
        for (int a = 0; a < QPT; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j) cs[a][j] = f32x2{0.f, 0.f};
#pragma unroll
        for (int c = 0; c < S; ++c) {
            const float4 b = trow[c];
            const f32x2 b01{b.x, b.y}, b23{b.z, b.w};
            const int o = (c & 1) * 2;  // support_func.h:140-147
#pragma unroll
            for (int a = 0; a < QPT; ++a) {
                cs[a][o + 0] = cs[a][o + 0] + b01 * f32x2{q[a][c].x, q[a][c].y};
                cs[a][o + 1] = cs[a][o + 1] + b23 * f32x2{q[a][c].z, q[a][c].w};
            }
        }
#pragma unroll
        for (int a = 0; a < QPT; ++a) {
            const f32x2 m01 = cs[a][2] + cs[a][0], m23 = cs[a][3] + cs[a][1];  // :148 hi half onto lo half
            dist[a] = -((m01.x + m01.y) + (m23.x + m23.y));                     // :160-162
        }
    }
