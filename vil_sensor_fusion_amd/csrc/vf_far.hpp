// vf_far.hpp -- the whole account of the far between factors' rows (View::x_* and View::xl_*): how a slot resolves to keyframes
// (far_ref, far_cols, far_col, far_jac, far_res) and the four things kernels do with a slot's six rows -- scatter one into an
// increment-shaped buffer (far_scatter), add U^T u (far_ends, far_jt_apply), stage them in LDS (far_stage).  Users: vf_kernels.hip
// (kernels/far.inc: linearisation, gradient, Woodbury columns and their combine; kernels/k4_selinv_far.inc: the marginals' low-rank
// downdate) and vf_refine.hip (the rows of J the far factors add to the operator).  Not k_marginalize<FAR>: the joint marginalisation
// of an anchor builds its own W with folded columns from View::x_*, a different object.
// Included inside namespace vf after VF_DI is defined.
#pragma once
struct FarRef { int kind, idx, a, kb, nl; };
VF_DI FarRef far_ref(const View& v, int w, int s) {
    FarRef f{-1, 0, 0, 0, 0};
    const int nl = v.xl_n[w], lo = v.lo[w], hi = v.hi[w];
    if (s < nl) {
        if (hi - lo > 3 && v.mp_on[w]) { f.kind = 1; f.idx = s; f.a = lo; f.kb = v.xl_b[w * v.x_max + s]; f.nl = nl; }
    } else if (s - nl < v.x_max) {
        const int i = w * v.x_max + s - nl, a = v.x_a[i], kb = v.x_b[i];
        if (!(a < lo || kb >= hi || a >= kb)) { f.kind = 0; f.idx = s - nl; f.a = a; f.kb = kb; }
    }
    return f;
}
// The robust loss of entry i = w * x_max + index of the nonlinear lists (engines with View::x_loss only; DESIGN.md "4i"): the arrays
// sit in the allocation of x_in behind its [B][x_max] records -- the parameters k, [B][x_max] doubles, then the ids, [B][x_max]
// ints (far_loss_k_at, far_loss_id_at: vf_kernels.hpp, where the host that makes and fills them finds the same offsets) -- and this
// is the one device-side reader.
struct FarLoss { int loss; double k; };
VF_DI FarLoss far_loss(const View& v, int i) {
    const size_t n = (size_t)v.B * v.x_max;
    return {reinterpret_cast<const int*>(v.x_in + far_loss_id_at(n))[i], v.x_in[far_loss_k_at(n) + i]};
}
VF_DI int far_cols(const FarRef& f) { return f.kind == 1 ? 27 + 6 * f.nl : 12; }
// column c of a slot's six rows -> (window-local keyframe, dof of its 15)
VF_DI void far_col(const View& v, int w, const FarRef& f, int c, int& k, int& d) {
    if (f.kind == 1) {
        if (c < 15) { k = f.a; d = c; }
        else if (c < 21) { k = f.a + 1; d = c - 15; }
        else if (c < 27) { k = f.a + 2; d = c - 21; }
        else { const int e = (c - 27) / 6; k = v.xl_b[w * v.x_max + e]; d = c - 27 - 6 * e; }
    } else if (c < 6) { k = f.a; d = c; }
    else { k = f.kb; d = c - 6; }
}
// entry (row j, column c) of the whitened Jacobian / residual j, at the states of buffer `buf`
VF_DI double far_jac(const View& v, int w, const FarRef& f, int buf, int j, int c) {
    if (f.kind == 1) return v.xl_U[((size_t)w * 6 * v.x_max + 6 * f.idx + j) * xl_ld(v) + c];
    return v.x_out[(((size_t)buf * v.B + w) * v.x_max + f.idx) * BTW_OUT + 6 + (c < 6 ? 0 : 36) + j * 6 + (c < 6 ? c : c - 6)];
}
VF_DI double far_res(const View& v, int w, const FarRef& f, int buf, int j) {
    if (f.kind == 1) return v.xl_out[((size_t)buf * v.B + w) * 6 * v.x_max + 6 * f.idx + j];
    return v.x_out[(((size_t)buf * v.B + w) * v.x_max + f.idx) * BTW_OUT + j];
}
constexpr int FAR_NCMAX = 27 + 6 * MAX_EXTRA_BIG;      // the most columns a slot has
// Row j of slot f added into dst, increment-shaped with (keyframe k, dof d) at (k * 15 + d) * stride, column after column: columns
// that land on the same cell add up in column order.  GUARD: a column outside the window is left out (k is never outside the
// window -- far_ref gives such a slot kind -1 -- so the test cannot change a bit: for a dst that is not a whole window's)
template <bool GUARD>
VF_DI void far_scatter(const View& v, int w, const FarRef& f, int buf, int j, double* dst, size_t stride) {
    const int lo = v.lo[w], hi = v.hi[w], nc = f.kind >= 0 ? far_cols(f) : 0;
    for (int c = 0; c < nc; c++) {
        int k, d;
        far_col(v, w, f, c, k, d);
        if (!GUARD || (k >= lo && k < hi)) dst[((size_t)k * 15 + d) * stride] += far_jac(v, w, f, buf, j, c);
    }
}
// The far ends of window w's linear far factor (every linear slot's columns 27.. lie on them) into kb_l[MAX_EXTRA_BIG] in LDS, for
// far_jt_apply; by every lane of the workgroup
VF_DI void far_ends(const View& v, int w, int lane, int* kb_l) {
    if (lane < v.x_max) kb_l[lane] = v.xl_b[w * v.x_max + lane];
    __syncthreads();
}
// out += (the six rows of slot f)^T u by a workgroup of 64 lanes, u(r) the r-th of the six values; out is [G][15].  One lane per
// column; two far ends of a linear far factor may be the same keyframe, so the lane of the FIRST of the columns that land on one
// (keyframe, dof) adds them all, in increasing order, and the others add nothing.  Every lane of the workgroup calls it (a barrier
// behind each group of 64 columns); slots are applied one after the other, as two of them may touch the same keyframe.
template <class U>
VF_DI void far_jt_apply(const View& v, int w, const FarRef& f, int buf, int lane, const int* kb_l, U&& u, double* out) {
    const int nc = f.kind >= 0 ? far_cols(f) : 0;
    for (int c0 = 0; c0 < nc; c0 += 64) {
        const int c = c0 + lane;
        if (c < nc) {
            int k, d;
            far_col(v, w, f, c, k, d);
            double acc = 0.0;
            for (int r = 0; r < 6; r++) acc = fma(far_jac(v, w, f, buf, r, c), u(r), acc);
            bool first = true;                   // of the columns that land on this (keyframe, dof): far-end columns only
            if (f.kind == 1 && c >= 27)
                for (int c2 = 27 + d; c2 < nc; c2 += 6) {
                    if (c2 == c || kb_l[(c2 - 27) / 6] != k) continue;
                    if (c2 < c) { first = false; break; }
                    for (int r = 0; r < 6; r++) acc = fma(far_jac(v, w, f, buf, r, c2), u(r), acc);
                }
            if (first) out[((size_t)w * v.M + k) * 15 + d] += acc;
        }
        __syncthreads();
    }
}
// The six rows of slot f staged in LDS by a workgroup of nt threads: J[j * FAR_NCMAX + c] and the column's offset in an
// increment-shaped window, off[c] = k * 15 + d (GUARD: -1 outside the window, which never happens, as in far_scatter).  Returns
// the slot's columns; the barriers around it are the caller's.
template <bool GUARD>
VF_DI int far_stage(const View& v, int w, const FarRef& f, int buf, int tid, int nt, double* J, int* off) {
    const int nc = f.kind >= 0 ? far_cols(f) : 0;
    for (int c = tid; c < nc; c += nt) {
        int k, d;
        far_col(v, w, f, c, k, d);
        off[c] = !GUARD || (k >= v.lo[w] && k < v.hi[w]) ? k * 15 + d : -1;
        for (int j = 0; j < 6; j++) J[j * FAR_NCMAX + c] = far_jac(v, w, f, buf, j, c);
    }
    return nc;
}
