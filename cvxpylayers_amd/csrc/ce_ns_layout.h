// ce_ns_layout.h -- the dynamic-LDS layout of k_backward_ns (ce_backward_ns.h) as data: offset and length of every segment and the footprint.  The host plans on
// its total (ce_plan.h plan_engine) and tests/test_ns_layout_host.py compiles it with plain g++; the kernel still carves by pointer bumping (its code is
// untouched), segment for segment in the order below.  No device intrinsics; a translation unit without the HIP headers defines __host__ and __device__ away
// before including it.
#pragma once          // (size_t: the including translation unit has <cstddef> or the HIP headers)

// pitch of the sweep's row buffers: 16 mod 32 doubles (conflict-free) with at least 16 doubles of gap behind the 16 NTILE entries of a row (the gaps of the
// eight buffer rows hold the ORIGINAL diagonal of the reduced Hessian: the rank tolerance of a pivot is relative to its own diagonal entry)
__host__ __device__ constexpr int bwd_ns_ldp(int NTILE) { return (16 * NTILE + 16) % 32 == 16 ? 16 * NTILE + 16 : 16 * NTILE + 32; }
__host__ __device__ constexpr int bwd_ns_kwmax(int m) { return ((m + 4) & ~3) + 4; }                                         // capacity of the weighted-row list (<= m entries + at least one pad, a multiple of 4;
                                                                                                                             // a triple adds at most its three rotated rows: still <= m)
__host__ __device__ constexpr int bwd_ns_nsl(int NTILE) { return (16 * NTILE - 3 + 63) / 64; }                               // 64-lane slots that hold the columns 0 .. n (n = right-hand side)

// doubles of the union region: {a_z, the row elimination's two publication buffers} | the sweep's row buffers | {q, g}   (nqs = max(nq, 1); the kernel's carve uses it)
__host__ __device__ constexpr int bwd_ns_union_doubles(int n, int m, int nqs, int NTILE) {
    const int npad = n + (n & 1);
    const int a = nqs * npad + 2 * (64 * bwd_ns_nsl(NTILE) + 2), b = 8 * bwd_ns_ldp(NTILE), c = m + (m & 1) + npad;
    const int r = a > b ? a : b;
    return r > c ? r : c;
}

// a segment: first element and element count, in doubles from sm for the double segments, in ints from (int *)sm for the int segments
struct NsSeg { int off, len; };
struct NsLayout {
    // ---- doubles
    NsSeg A;         // the instance's A, dense solver form, pitch n (the host sets DevT::lda = n for this family)
    NsSeg vv;        // v = y - s ; later r_y
    NsSeg dv;        // dy, then d = DPi dy ; later y (outputs)
    NsSeg rx;
    NsSeg fvec;      // f = dx + sum over boundary cones [...]; its free entries become Z^T f ; later x (outputs)
    NsSeg dB;        // right-hand side of the equalities -> d~ -> x_piv ; finally the multipliers mu
    NsSeg cinfo;     // per cone: lambda, |z|, e_y.d, e_s.d, theta
    NsSeg tvec;      // per weighted row: t_k = a_k . x_p ; later q_k = a_k . r_x
    NsSeg wgt;       // per weighted row: its weight in H (theta_c for the z-rows of cone c, -theta_c for a_z)
    NsSeg red;       // refinement: the partial maxima of the residual norms, two per wave
    NsSeg qaz;       // a_z . r_x per cone
    NsSeg U;         // the union region (16-byte aligned); its members, each alive in its own phase:
    NsSeg az;        //   a_z = A_z^T z-hat per boundary cone (pitch npad); dead after the Gram
    NsSeg pub;       //   row elimination: two publication buffers {scaled pivot row (64 NSL), inverse pivot, pivot column}
    NsSeg Rbuf;      //   the sweep's two buffers of four rows
    NsSeg qv2;       //   (A r_x)_i for the rows of boundary cones, after the sweep
    NsSeg mu;        //   g = (H r_x - f)[piv] by equality index, after the sweep (the multipliers themselves end in dB)
    // ---- ints
    NsSeg rkind, eqrow, ckind, ceq;
    NsSeg cbase;     // first entry of cone c in the weighted-row list
    NsSeg erow;      // equality e -> offset of its row in sm
    NsSeg pcol;      // equality e -> pivot column (-1: redundant row, dropped)
    NsSeg cmap;      // column j -> free index f (>= 0) or -1 (pivot column)
    NsSeg fcol;      // free index f -> column ; before the row elimination: equality e -> source (row index >= 0, or -1 - cone)
    NsSeg wrow;      // weighted row -> offset of its row in sm
    NsSeg wsrc;      // weighted row -> row index of A (>= 0) or -1 - cone (a_z)
    NsSeg wcnt;
    NsSeg misc;      // [0] n_eq, [1] nf, [2] flags, [3] KW
    // ---- quadratic objective only (len 0 otherwise), behind the ints rounded to 8 bytes
    NsSeg Pm;        // doubles: P, dense and symmetric (pitch n); step 2 turns its rows into p~_j = Z^T p_j in the free columns
    NsSeg ptv;       // doubles: per row of P, t_j = p_j . x_p
    NsSeg peq;       // ints: pivot column j -> its equality e
    // ---- exponential / power triples only (TRI mode; len 0 otherwise), behind the ints rounded to 8 bytes
    NsSeg Wt;        // doubles: per triple the eigenvectors W (row-major 3 x 3, columns) of D Pi_K*(v): the triple's rows of A are rotated by W^T in place
    NsSeg lamt;      // doubles: per rotated triple row its eigenvalue lambda after the snap (1: equality, 0: dropped, else a weighted row)
    // ---- PSD blocks only (PSD mode; len 0 otherwise), behind the ints rounded to 8 bytes.  NONE of them aliases the union region or any other segment: U, Lambda
    //      and B live from the decomposition to the rotation back in the epilogue, across every phase of the union's members; the two scratch segments are used in
    //      the classification pass, in the epilogue and in the refinement's projections, and cost 5.2 KB at order 8 with four waves -- kept apart, no phase proof needed
    NsSeg psdU;      // doubles: per block the eigenvectors U of smat(v_c) (row-major, pitch maxs x maxs per block, order k x k inside, vectors in the columns)
    NsSeg psdEv;     // doubles: per block its eigenvalues Lambda (pitch maxs)
    NsSeg lamp;      // doubles: per rotated PSD row (a, b) the eigenvalue B_ab of D Pi (1: equality, 0: dropped, else a weighted row)
    NsSeg psdScr;    // doubles: the Jacobi scratch, 2 maxs^2 + 2 maxs + 8 (ce_psd_jacobi.h: S, a spare matrix, the rotations of a round)
    NsSeg psdXW;     // doubles: the rotation's (X, W) pair of maxs x maxs matrices per wave
    // ---- ints: the footprint has always counted the two alignment doubles (behind A, in front of U) whether or not the carve takes them, and the launch plan
    //      is decided on the footprint: the ones not taken stay reserved here, at the end (two ints each), and nothing uses them
    NsSeg slack;
    size_t bytes;    // the footprint: the end of the last segment
};

// the modes of the layout: the plain one, the one with the dense P behind the ints (qp), the one with the triples' segments there (ntri > 0 triples; never with qp),
// the one with the PSD blocks' segments there (ns > 0 blocks of order <= maxs that own psdrows rows together; never with qp), and the one with both cone kinds
// (ntri > 0 and ns > 0: the triples' two segments, then the blocks' five, no segment of its own)
__host__ __device__ constexpr NsLayout ns_layout(int n, int m, int nq, int NTILE, int NTHR, bool qp, int ntri = 0, int ns = 0, int maxs = 0, int psdrows = 0) {
    const int nqs = nq > 0 ? nq : 1, npad = n + (n & 1), kw = bwd_ns_kwmax(m), nwb = NTHR / 64;
    NsLayout L{};
    int p = 0, taken = 0;          // doubles
    L.A = {p, m * n}; p += m * n; taken += p & 1; p += p & 1;
    L.vv = {p, m}; p += m;
    L.dv = {p, m}; p += m;
    L.rx = {p, npad}; p += npad;
    L.fvec = {p, npad}; p += npad;
    L.dB = {p, npad}; p += npad;
    L.cinfo = {p, 5 * nqs}; p += 5 * nqs;
    L.tvec = {p, kw}; p += kw;
    L.wgt = {p, kw}; p += kw;
    L.red = {p, nwb * 8}; p += nwb * 8;
    L.qaz = {p, nqs}; p += nqs;
    taken += p & 1; p += p & 1;
    L.az = {p, nqs * npad};
    L.pub = {p + nqs * npad, 2 * (64 * bwd_ns_nsl(NTILE) + 2)};
    L.Rbuf = {p, 8 * bwd_ns_ldp(NTILE)};
    L.qv2 = {p, m + (m & 1)};
    L.mu = {p + m + (m & 1), npad};
    const int u = bwd_ns_union_doubles(n, m, nqs, NTILE);
    L.U = {p, u}; p += u;
    int ip = 2 * p;                // ints
    L.rkind = {ip, m}; ip += m;
    L.eqrow = {ip, m}; ip += m;
    L.ckind = {ip, nqs}; ip += nqs;
    L.ceq = {ip, nqs}; ip += nqs;
    L.cbase = {ip, nqs}; ip += nqs;
    L.erow = {ip, n}; ip += n;
    L.pcol = {ip, n}; ip += n;
    L.cmap = {ip, n}; ip += n;
    L.fcol = {ip, n}; ip += n;
    L.wrow = {ip, kw}; ip += kw;
    L.wsrc = {ip, kw}; ip += kw;
    L.wcnt = {ip, nwb + 1}; ip += nwb + 1;
    L.misc = {ip, 8}; ip += 8;
    L.Pm = {0, 0}; L.ptv = {0, 0}; L.peq = {0, 0};
    if (qp) {
        ip += ip & 1;
        p = ip / 2;
        L.Pm = {p, n * n}; p += n * n;
        L.ptv = {p, npad}; p += npad;
        ip = 2 * p;
        L.peq = {ip, n}; ip += n;
    }
    L.Wt = {0, 0}; L.lamt = {0, 0};
    if (ntri > 0) {
        ip += ip & 1;
        p = ip / 2;
        L.Wt = {p, 9 * ntri}; p += 9 * ntri;
        L.lamt = {p, 3 * ntri}; p += 3 * ntri;
        ip = 2 * p;
    }
    L.psdU = {0, 0}; L.psdEv = {0, 0}; L.lamp = {0, 0}; L.psdScr = {0, 0}; L.psdXW = {0, 0};
    if (ns > 0) {
        ip += ip & 1;
        p = ip / 2;
        L.psdU = {p, ns * maxs * maxs}; p += ns * maxs * maxs;
        L.psdEv = {p, ns * maxs}; p += ns * maxs;
        L.lamp = {p, psdrows}; p += psdrows;
        L.psdScr = {p, 2 * maxs * maxs + 2 * maxs + 8}; p += 2 * maxs * maxs + 2 * maxs + 8;
        L.psdXW = {p, 2 * nwb * maxs * maxs}; p += 2 * nwb * maxs * maxs;
        ip = 2 * p;
    }
    L.slack = {ip, 2 * (2 - taken)}; ip += 2 * (2 - taken);
    L.bytes = (size_t)ip * 4;
    return L;
}
// what the launch plan asks for (ce_plan.h plan_engine)
__host__ __device__ constexpr size_t bwd_ns_lds_bytes_of(int n, int m, int nq, int NTILE, int NTHR) { return ns_layout(n, m, nq, NTILE, NTHR, false).bytes; }
__host__ __device__ constexpr size_t bwd_ns_qp_lds_bytes_of(int n, int m, int nq, int NTILE, int NTHR) { return ns_layout(n, m, nq, NTILE, NTHR, true).bytes; }
__host__ __device__ constexpr size_t bwd_ns_tri_lds_bytes_of(int n, int m, int nq, int ntri, int NTILE, int NTHR) { return ns_layout(n, m, nq, NTILE, NTHR, false, ntri).bytes; }
__host__ __device__ constexpr size_t bwd_ns_psd_lds_bytes_of(int n, int m, int nq, int ns, int maxs, int psdrows, int NTILE, int NTHR) { return ns_layout(n, m, nq, NTILE, NTHR, false, 0, ns, maxs, psdrows).bytes; }
__host__ __device__ constexpr size_t bwd_ns_psd_tri_lds_bytes_of(int n, int m, int nq, int ntri, int ns, int maxs, int psdrows, int NTILE, int NTHR) { return ns_layout(n, m, nq, NTILE, NTHR, false, ntri, ns, maxs, psdrows).bytes; }
