// t4d_priors.hip — the topology priors of Topo4D's geometry loop (get_loss, train.py:328-368), forward and backward, on the raw
// parameters, in two launches per evaluation:
//
//  * k_priors_elements (phase A): one thread per element of one term - a (Gaussian, neighbour slot) pair for rigid / rot / iso, a
//    Gaussian for scale / scale_max, an interior edge for the flatten terms, a region vertex for FlattenLoss_v2.  It evaluates the
//    element's weighted loss and writes its local gradient contributions, each to a record of its own (no atomics), and one loss
//    partial per block and term.
//  * k_priors_vertices (phase B): one thread per vertex gathers the records that name it - its own K neighbour slots, the slots of
//    other Gaussians that name it (transposed neighbour list), and the flatten records (CSR) - in a fixed order, every term into a
//    sum of its own and the terms' sums added last, then applies the chain rule through quat_mult, normalize and exp (per term
//    for the quaternion) and writes (or adds) the three raw gradients.  Block 0 also reduces the loss
//    partials, term by term in block order.
//
// Fixed summation orders everywhere: the result is bit-identical from run to run.  The arithmetic restates the reference's
// formulas (helpers.py:126-144, external.py:26-43, loss_util.py FlattenLoss / FlattenLoss_v2 / SoftFlattenLoss) with torch's
// derivative conventions: abs'(0) = relu'(0) = 0, acos unclamped, the min / max gradient to the index torch returns.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/topo4d_raster.h"
#include "t4d_block.h"
#include "t4d_host.h"

namespace {

constexpr int kBlock = 256;          // 4 wave64s: the elements are independent, short and latency-bound
constexpr int kMaxSegs = 12;
constexpr int kNbrTerms = 3;         // partial slots per block (rigid, rot, iso share a segment)

enum SegKind { SEG_NBR, SEG_SCALE, SEG_EDGE, SEG_REGION };

struct Seg {
    int kind, term, n, block0, sub;   // sub: edge / region index; term: first T4D_PRIOR_* the segment reduces into
    int64_t rec_base;                 // first position record (edge / region segments)
    float coef;                       // weight / the reference's denominator (mean over P*K, MSE over 3 R, sum: 1)
};

struct Segs {
    Seg s[kMaxSegs];
    int n, blocks;
    float coef_nbr[kNbrTerms];        // rigid, rot, iso
};

struct Ptr {
    const float *x, *q, *ls;
    float4 *posR, *posI, *rotR, *rotQ, *rec, *scale_g;   // rigid / iso offset gradients, rigid / rot rel_rot gradients per (g, k)
    float *partial;
};

__device__ __forceinline__ float3 ld3(const float *p, int i) { return make_float3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
__device__ __forceinline__ float4 ld4(const float *p, int i) { return *reinterpret_cast<const float4 *>(p + 4 * (size_t)i); }
__device__ __forceinline__ float3 sub3(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float3 add3(float3 a, float3 b) { return make_float3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ float3 mul3(float3 a, float s) { return make_float3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot3(float3 a, float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// torch.nn.functional.normalize: x / max(||x||, 1e-12)
__device__ __forceinline__ float4 normalize4(float4 q, float &den)
{
    den = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);
    return make_float4(q.x / den, q.y / den, q.z / den, q.w / den);
}

// helpers.quat_mult(q1, q2), (w, x, y, z) in (.x, .y, .z, .w)
__device__ __forceinline__ float4 quat_mult(float4 a, float4 b)
{
    return make_float4(a.x * b.x - a.y * b.y - a.z * b.z - a.w * b.w, a.x * b.y + a.y * b.x + a.z * b.w - a.w * b.z,
                       a.x * b.z - a.y * b.w + a.z * b.x + a.w * b.y, a.x * b.w + a.y * b.z - a.z * b.y + a.w * b.x);
}

// d quat_mult(a, b) / d a, transposed, applied to g
__device__ __forceinline__ float4 quat_mult_bwd_a(float4 b, float4 g)
{
    return make_float4(b.x * g.x + b.y * g.y + b.z * g.z + b.w * g.w, -b.y * g.x + b.x * g.y - b.w * g.z + b.z * g.w,
                       -b.z * g.x + b.w * g.y + b.x * g.z - b.y * g.w, -b.w * g.x - b.z * g.y + b.y * g.z + b.x * g.w);
}

__device__ __forceinline__ float4 rel_rot(const float *q, const float *pinv, int i)
{
    float den;
    return quat_mult(normalize4(ld4(q, i), den), ld4(pinv, i));
}

// ---- SoftFlattenLoss / FlattenLoss geometry of one interior edge (v0, v1) with opposite vertices v2, v3 --------------------
struct Side {   // one of the two triangles: b = v2 - v0 (or v3 - v0)
    float al2, bl2, al1, bl1, ab, M, cosi, sin, r;
    float3 b, cb;
};

__device__ __forceinline__ Side side_fwd(float3 a, float3 b)
{
    const float eps = 1e-6f;
    Side s;
    s.b = b;
    s.al2 = dot3(a, a);
    s.bl2 = dot3(b, b);
    s.al1 = sqrtf(s.al2 + eps);
    s.bl1 = sqrtf(s.bl2 + eps);
    s.ab = dot3(a, b);
    s.M = s.al1 * s.bl1 + eps;
    s.cosi = s.ab / s.M;
    s.sin = sqrtf(1.f - s.cosi * s.cosi + eps);
    s.r = s.ab / (s.al2 + eps);
    s.cb = sub3(b, mul3(a, s.r));
    return s;
}

// adjoint of one side: (gcb, gcbl1) -> accumulates ga, returns gb
__device__ __forceinline__ float3 side_bwd(const Side &s, float3 a, float3 gcb, float gcbl1, float3 &ga)
{
    const float eps = 1e-6f;
    float gbl1 = gcbl1 * s.sin;
    const float gsin = gcbl1 * s.bl1;
    float3 gb = gcb;                                     // cb = b - c
    const float3 gc = mul3(gcb, -1.f);
    ga = add3(ga, mul3(gc, s.r));                        // c = a * r
    const float gr = dot3(gc, a);
    const float den = s.al2 + eps;
    float gab = gr / den;
    float gal2 = -gr * s.ab / (den * den);
    const float gcos = gsin * (-s.cosi) / s.sin;         // sin = sqrt(1 - cos^2 + eps)
    gab += gcos / s.M;                                   // cos = ab / M
    const float gM = -gcos * s.ab / (s.M * s.M);
    const float gal1 = gM * s.bl1;
    gbl1 += gM * s.al1;
    gal2 += gal1 / (2.f * s.al1);
    const float gbl2 = gbl1 / (2.f * s.bl1);
    ga = add3(ga, add3(mul3(a, 2.f * gal2), mul3(s.b, gab)));
    gb = add3(gb, add3(mul3(s.b, 2.f * gbl2), mul3(a, gab)));
    return gb;
}

// Block reduction of kNbrTerms values in a fixed order (xor butterflies in a wave, then the four waves in order)
__device__ __forceinline__ void block_partials(float v[kNbrTerms], float *out)
{
    __shared__ float w[kNbrTerms][kBlock / 64];
#pragma unroll
    for (int t = 0; t < kNbrTerms; t++) {
        const float s = wave_sum(v[t]);
        if ((threadIdx.x & 63) == 0) w[t][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x < kNbrTerms) out[threadIdx.x] = (w[threadIdx.x][0] + w[threadIdx.x][1]) + (w[threadIdx.x][2] + w[threadIdx.x][3]);
}

__global__ __launch_bounds__(kBlock) void k_priors_elements(const T4DPriors pr, const Segs S, const Ptr p, const int is_initial)
{
    int si = 0;
    while (si + 1 < S.n && (int)blockIdx.x >= S.s[si + 1].block0) si++;
    const Seg sg = S.s[si];
    const int i = ((int)blockIdx.x - sg.block0) * kBlock + threadIdx.x;
    float v[kNbrTerms] = {0.f, 0.f, 0.f};
    if (i < sg.n) {
        if (sg.kind == SEG_NBR) {
            // element (g, k): rigid, rot, iso of train.py:330-346
            const int g = i / pr.K, e = i;
            const int n = pr.nbr[e];
            const float3 xg = ld3(p.x, g), xn = ld3(p.x, n);
            const float4 rg = rel_rot(p.q, pr.prev_inv_rot, g), rn = rel_rot(p.q, pr.prev_inv_rot, n);
            const float3 off = sub3(xn, xg);
            // build_rotation (external.py:26-43) normalises rel_rot again, without an epsilon
            const float nq = sqrtf(rg.x * rg.x + rg.y * rg.y + rg.z * rg.z + rg.w * rg.w);
            const float r = rg.x / nq, x = rg.y / nq, y = rg.z / nq, z = rg.w / nq;
            const float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
                                   {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
                                   {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
            // rigid: || R^T off - prev_offset ||, weighted_l2_loss_v2 (helpers.py:130-131)
            const float3 po = ld3(pr.prev_offset, e);
            const float3 vr = make_float3(R[0][0] * off.x + R[1][0] * off.y + R[2][0] * off.z,
                                          R[0][1] * off.x + R[1][1] * off.y + R[2][1] * off.z,
                                          R[0][2] * off.x + R[1][2] * off.y + R[2][2] * off.z);
            const float3 d = sub3(vr, po);
            const float wr = pr.rig_w[e];
            const float s1 = sqrtf(dot3(d, d) * wr + 1e-20f);
            v[0] = s1 * S.coef_nbr[0];
            const float3 gv = mul3(d, S.coef_nbr[0] * wr / s1);
            const float3 goff = make_float3(R[0][0] * gv.x + R[0][1] * gv.y + R[0][2] * gv.z, R[1][0] * gv.x + R[1][1] * gv.y + R[1][2] * gv.z,
                                      R[2][0] * gv.x + R[2][1] * gv.y + R[2][2] * gv.z);
            // dL/dR[j][i] = gv_i off_j, then through the matrix entries to (r, x, y, z)
            const float o[3] = {off.x, off.y, off.z}, gvv[3] = {gv.x, gv.y, gv.z};
            float G[3][3];
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int c = 0; c < 3; c++) G[j][c] = gvv[c] * o[j];
            const float gr_ = 2.f * (-z * G[0][1] + y * G[0][2] + z * G[1][0] - x * G[1][2] - y * G[2][0] + x * G[2][1]);
            const float gx_ = 2.f * (y * G[0][1] + z * G[0][2] + y * G[1][0] - 2.f * x * G[1][1] - r * G[1][2] + z * G[2][0] + r * G[2][1] -
                                     2.f * x * G[2][2]);
            const float gy_ = 2.f * (-2.f * y * G[0][0] + x * G[0][1] + r * G[0][2] + x * G[1][0] + z * G[1][2] - r * G[2][0] + z * G[2][1] -
                                     2.f * y * G[2][2]);
            const float gz_ = 2.f * (-2.f * z * G[0][0] - r * G[0][1] + x * G[0][2] + r * G[1][0] - 2.f * z * G[1][1] + y * G[1][2] +
                                     x * G[2][0] + y * G[2][1]);
            const float pd = r * gr_ + x * gx_ + y * gy_ + z * gz_;
            const float4 grg = make_float4((gr_ - r * pd) / nq, (gx_ - x * pd) / nq, (gy_ - y * pd) / nq, (gz_ - z * pd) / nq);
            // rot: || rel_rot[nbr] - rel_rot ||, weighted_l2_loss_v2
            const float4 dq = make_float4(rn.x - rg.x, rn.y - rg.y, rn.z - rg.z, rn.w - rg.w);
            const float wq = pr.rot_w[e];
            const float s2 = sqrtf((dq.x * dq.x + dq.y * dq.y + dq.z * dq.z + dq.w * dq.w) * wq + 1e-20f);
            v[1] = s2 * S.coef_nbr[1];
            const float c2 = S.coef_nbr[1] * wq / s2;
            const float4 grn = make_float4(dq.x * c2, dq.y * c2, dq.z * c2, dq.w * c2);
            // iso: | sqrt(|off|^2 + 1e-20) - neighbor_dist |, weighted_l2_loss_v1 (helpers.py:126-127)
            const float mag = sqrtf(dot3(off, off) + 1e-20f);
            const float rd = mag - pr.nbr_dist[e];
            const float wi = pr.iso_w[e];
            const float s3 = sqrtf(rd * rd * wi + 1e-20f);
            v[2] = s3 * S.coef_nbr[2];
            const float3 giso = mul3(off, S.coef_nbr[2] * wi * rd / s3 / mag);
            // one record per term: the neighbour receives it, the Gaussian its negative (rot: rel_rot[nbr] - rel_rot likewise)
            p.posR[e] = make_float4(goff.x, goff.y, goff.z, 0.f);
            p.posI[e] = make_float4(giso.x, giso.y, giso.z, 0.f);
            p.rotR[e] = grg;
            p.rotQ[e] = grn;
        } else if (sg.kind == SEG_SCALE) {
            // scale = sum_g min_c exp(ls), scale_max = sum_g relu(max_c exp(ls) - 1.5 init_scale) (train.py:360-363).
            // Tie rule: torch.min / torch.max over dim 1 return the FIRST index of the extreme value (the CPU golden shows the
            // gradient of a row of three equal scales in column 0 only): strict comparisons, scanned from column 0.
            const float s0 = expf(p.ls[3 * i]), s1 = expf(p.ls[3 * i + 1]), s2 = expf(p.ls[3 * i + 2]);
            const float sc[3] = {s0, s1, s2};
            int imin = 0, imax = 0;
            for (int c = 1; c < 3; c++) {
                if (sc[c] < sc[imin]) imin = c;
                if (sc[c] > sc[imax]) imax = c;
            }
            const float cs = S.s[si].coef, cm = pr.weights[T4D_PRIOR_SCALE_MAX];
            v[0] = sc[imin] * cs;
            const float m = sc[imax] - pr.init_scale[i] * 1.5f;
            v[1] = (m > 0.f ? m : 0.f) * cm;
            float g3[3] = {0.f, 0.f, 0.f};
            g3[imin] += cs * sc[imin];
            if (m > 0.f) g3[imax] += cm * sc[imax];
            p.scale_g[i] = make_float4(g3[0], g3[1], g3[2], 0.f);
        } else if (sg.kind == SEG_EDGE) {
            const int32_t *E = pr.edges[sg.sub];
            const int ne = pr.n_edges[sg.sub];
            const int i0 = E[i], i1 = E[ne + i], i2 = E[2 * ne + i], i3 = E[3 * ne + i];
            const float3 x0 = ld3(p.x, i0);
            const float3 a = sub3(ld3(p.x, i1), x0);
            const Side A = side_fwd(a, sub3(ld3(p.x, i2), x0));
            const Side B = side_fwd(a, sub3(ld3(p.x, i3), x0));
            const float c1 = A.bl1 * A.sin, c2 = B.bl1 * B.sin;
            const float D = dot3(A.cb, B.cb), Q = c1 * c2 + 1e-6f;
            const float cosv = D / Q;
            const int soft = sg.sub >= 2;                    // edge terms 2..5 are the SoftFlattenLoss ones
            float L, gcos;
            if (!soft) {
                // FlattenLoss, threshold 0: torch.where(cos > cos(0) = 1, -1, cos), then (cos + 1)^2
                const bool out = cosv > 1.f;
                L = out ? 0.f : (cosv + 1.f) * (cosv + 1.f);
                gcos = out ? 0.f : 2.f * (cosv + 1.f);
            } else if (is_initial) {
                pr.cos_init[sg.sub - 2][i] = cosv;           // the cos_init of the later frames (train.py:365-368)
                L = (cosv + 1.f) * (cosv + 1.f);
                gcos = 2.f * (cosv + 1.f);
            } else {
                // 1 - cos(|acos(cos) - acos(cos_init)|); acos unclamped as torch's, abs'(0) = 0
                const float t = acosf(cosv) - acosf(pr.cos_init[sg.sub - 2][i]);
                L = 1.f - cosf(fabsf(t));
                const float sg_t = t > 0.f ? 1.f : (t < 0.f ? -1.f : (t == t ? 0.f : t));
                gcos = sinf(fabsf(t)) * sg_t * (-1.f / sqrtf(1.f - cosv * cosv));
            }
            v[0] = L * sg.coef;
            gcos *= sg.coef;
            const float gD = gcos / Q, gQ = -gcos * D / (Q * Q);
            float3 ga = make_float3(0.f, 0.f, 0.f);
            const float3 gb1 = side_bwd(A, a, mul3(B.cb, gD), gQ * c2, ga);
            const float3 gb2 = side_bwd(B, a, mul3(A.cb, gD), gQ * c1, ga);
            const float3 g0 = mul3(add3(add3(ga, gb1), gb2), -1.f);
            float4 *rec = p.rec + sg.rec_base + 4 * (int64_t)i;
            rec[0] = make_float4(g0.x, g0.y, g0.z, 0.f);
            rec[1] = make_float4(ga.x, ga.y, ga.z, 0.f);
            rec[2] = make_float4(gb1.x, gb1.y, gb1.z, 0.f);
            rec[3] = make_float4(gb2.x, gb2.y, gb2.z, 0.f);
        } else {
            // FlattenLoss_v2: MSE over region x 3 of (masked one-ring mean - vertex)
            const int vtx = pr.region[sg.sub][i];
            float3 sum = make_float3(0.f, 0.f, 0.f);
            for (int k = 0; k < pr.K; k++) sum = add3(sum, mul3(ld3(p.x, pr.nbr[vtx * pr.K + k]), pr.nbr_mask[vtx * pr.K + k]));
            const float nn = (float)pr.nbr_num[vtx];
            const float3 d = sub3(make_float3(sum.x / nn, sum.y / nn, sum.z / nn), ld3(p.x, vtx));
            v[0] = dot3(d, d) * sg.coef;
            const float3 gave = mul3(d, 2.f * sg.coef);
            float4 *rec = p.rec + sg.rec_base + (int64_t)(pr.K + 1) * i;
            for (int k = 0; k < pr.K; k++) {
                const float mk = pr.nbr_mask[vtx * pr.K + k];
                rec[k] = make_float4(gave.x / nn * mk, gave.y / nn * mk, gave.z / nn * mk, 0.f);
            }
            rec[pr.K] = make_float4(-gave.x, -gave.y, -gave.z, 0.f);
        }
    }
    block_partials(v, p.partial + kNbrTerms * (size_t)blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void k_priors_vertices(const T4DPriors pr, const Segs S, const Ptr p, const int is_initial,
                                                            float *dx, float *dq, float *dls, const float *upstream, const int accumulate,
                                                            float *losses)
{
    const int v = blockIdx.x * kBlock + threadIdx.x;
    const float up = upstream ? *upstream : 1.f;
    if (v < pr.P) {
        // Every term is summed on its own, in the order a one-term evaluation sums it, and the terms are added last: the gradient
        // of all terms is the rounded sum of the gradients of the terms alone, whatever cancels inside a term.
        float3 gx = make_float3(0.f, 0.f, 0.f);
        float4 qr = make_float4(0.f, 0.f, 0.f, 0.f), qo = qr;     // d rigid / d rel_rot, d rot / d rel_rot
        if (!is_initial) {
            float3 xr = make_float3(0.f, 0.f, 0.f), xi = xr;
            for (int k = 0; k < pr.K; k++) {
                const int e = v * pr.K + k;
                const float4 a = p.posR[e], c = p.posI[e], b = p.rotR[e], d = p.rotQ[e];
                xr = sub3(xr, make_float3(a.x, a.y, a.z));
                xi = sub3(xi, make_float3(c.x, c.y, c.z));
                qr = make_float4(qr.x + b.x, qr.y + b.y, qr.z + b.z, qr.w + b.w);
                qo = make_float4(qo.x - d.x, qo.y - d.y, qo.z - d.z, qo.w - d.w);
            }
            for (int j = pr.nbr_t_off[v]; j < pr.nbr_t_off[v + 1]; j++) {
                const int e = pr.nbr_t_idx[j];
                const float4 a = p.posR[e], c = p.posI[e], d = p.rotQ[e];
                xr = add3(xr, make_float3(a.x, a.y, a.z));
                xi = add3(xi, make_float3(c.x, c.y, c.z));
                qo = make_float4(qo.x + d.x, qo.y + d.y, qo.z + d.z, qo.w + d.w);
            }
            gx = add3(xr, xi);
        }
        // the flatten records of a vertex ascend, so they come term by term: a term's sum joins the total where the next one begins
        const int f = is_initial ? 0 : 1;
        int si = 0;
        while (si < S.n && S.s[si].kind != SEG_EDGE && S.s[si].kind != SEG_REGION) si++;
        float3 acc = make_float3(0.f, 0.f, 0.f);
        for (int j = pr.rec_off[f][v]; j < pr.rec_off[f][v + 1]; j++) {
            const int rid = pr.rec_idx[f][j];
            while (si + 1 < S.n && (int64_t)rid >= S.s[si + 1].rec_base) {
                gx = add3(gx, acc);
                acc = make_float3(0.f, 0.f, 0.f);
                si++;
            }
            const float4 a = p.rec[rid];
            acc = add3(acc, make_float3(a.x, a.y, a.z));
        }
        gx = add3(gx, acc);
        // rel_rot = quat_mult(normalize(q), prev_inv_rot): back through the product and the normalisation, term by term
        float4 gq = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!is_initial) {
            float den;
            const float4 rn = normalize4(ld4(p.q, v), den);
            const float4 pinv = ld4(pr.prev_inv_rot, v);
            const float4 grr[2] = {qr, qo};
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const float4 gn = quat_mult_bwd_a(pinv, grr[t]);
                const float pd = rn.x * gn.x + rn.y * gn.y + rn.z * gn.z + rn.w * gn.w;
                gq = make_float4(gq.x + (gn.x - rn.x * pd) / den, gq.y + (gn.y - rn.y * pd) / den, gq.z + (gn.z - rn.z * pd) / den,
                                 gq.w + (gn.w - rn.w * pd) / den);
            }
        }
        float3 gs = make_float3(0.f, 0.f, 0.f);
        if (is_initial) {
            const float4 s = p.scale_g[v];
            gs = make_float3(s.x, s.y, s.z);
        }
        const float o3[3] = {gx.x * up, gx.y * up, gx.z * up}, s3[3] = {gs.x * up, gs.y * up, gs.z * up};
        const float q4[4] = {gq.x * up, gq.y * up, gq.z * up, gq.w * up};
        for (int c = 0; c < 3; c++) {
            dx[3 * v + c] = accumulate ? dx[3 * v + c] + o3[c] : o3[c];
            dls[3 * v + c] = accumulate ? dls[3 * v + c] + s3[c] : s3[c];
        }
        for (int c = 0; c < 4; c++) dq[4 * v + c] = accumulate ? dq[4 * v + c] + q4[c] : q4[c];
    }
    if (blockIdx.x != 0) return;
    // the loss partials: per term, the blocks of its segment in block order, lanes then waves in a fixed order
    __shared__ float acc[T4D_PRIORS_TERMS];
    __shared__ float w[kBlock / 64];
    if (threadIdx.x < T4D_PRIORS_TERMS) acc[threadIdx.x] = 0.f;
    __syncthreads();
    for (int si = 0; si < S.n; si++) {
        const Seg sg = S.s[si];
        const int nb = (sg.n + kBlock - 1) / kBlock;
        const int slots = sg.kind == SEG_NBR ? 3 : (sg.kind == SEG_SCALE ? 2 : 1);
        for (int t = 0; t < slots; t++) {
            float s = 0.f;
            for (int b = threadIdx.x; b < nb; b += kBlock) s += p.partial[kNbrTerms * (size_t)(sg.block0 + b) + t];
            s = wave_sum(s);
            if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
            __syncthreads();
            if (threadIdx.x == 0) acc[sg.term + t] = (w[0] + w[1]) + (w[2] + w[3]);
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        float tot = 0.f;
        for (int t = 0; t < T4D_PRIORS_TERMS; t++) {
            losses[t] = acc[t];
            tot += acc[t];
        }
        losses[T4D_PRIORS_TERMS] = tot;
    }
}

// edge terms in T4DPriors order -> loss slots; region terms likewise
constexpr int kEdgeTerm[T4D_PRIORS_EDGE_TERMS] = {T4D_PRIOR_FLAT, T4D_PRIOR_FLAT_LIP_BOTTOM, T4D_PRIOR_FLAT_LID_TOP,
                                                  T4D_PRIOR_FLAT_LID_BOTTOM, T4D_PRIOR_FLAT_LIP, T4D_PRIOR_FLAT_MOUTH};
constexpr int kRegionTerm[T4D_PRIORS_REGION_TERMS] = {T4D_PRIOR_FLAT_EYE, T4D_PRIOR_FLAT_FACE_BOTTOM, T4D_PRIOR_FLAT_LIP_SOCKET};

int64_t record_layout(const T4DPriors *pr, int64_t *base)
{
    int64_t n = 0;
    for (int t = 0; t < T4D_PRIORS_EDGE_TERMS; t++) {
        if (base) base[t] = n;
        n += 4 * (int64_t)pr->n_edges[t];
    }
    for (int r = 0; r < T4D_PRIORS_REGION_TERMS; r++) {
        if (base) base[T4D_PRIORS_EDGE_TERMS + r] = n;
        n += (int64_t)(pr->K + 1) * pr->n_region[r];
    }
    return n;
}

void add_seg(Segs &S, int kind, int term, int n, int sub, int64_t rec_base, float coef)
{
    if (n <= 0) return;
    Seg &s = S.s[S.n++];
    s.kind = kind; s.term = term; s.n = n; s.sub = sub; s.rec_base = rec_base; s.coef = coef; s.block0 = S.blocks;
    S.blocks += (n + kBlock - 1) / kBlock;
}

Segs make_segs(const T4DPriors *pr, int is_initial)
{
    Segs S;
    memset(&S, 0, sizeof(S));
    int64_t base[T4D_PRIORS_EDGE_TERMS + T4D_PRIORS_REGION_TERMS];
    record_layout(pr, base);
    const int PK = pr->P * pr->K;
    if (is_initial) {
        add_seg(S, SEG_SCALE, T4D_PRIOR_SCALE, pr->P, 0, 0, pr->weights[T4D_PRIOR_SCALE]);
        for (int t = 2; t < T4D_PRIORS_EDGE_TERMS; t++) add_seg(S, SEG_EDGE, kEdgeTerm[t], pr->n_edges[t], t, base[t], pr->weights[kEdgeTerm[t]]);
    } else {
        // weighted_l2_loss_v1 / _v2 are means over all P*K (Gaussian, slot) pairs, the padded slots included
        add_seg(S, SEG_NBR, T4D_PRIOR_RIGID, PK, 0, 0, 0.f);
        S.coef_nbr[0] = pr->weights[T4D_PRIOR_RIGID] / (float)PK;
        S.coef_nbr[1] = pr->weights[T4D_PRIOR_ROT] / (float)PK;
        S.coef_nbr[2] = pr->weights[T4D_PRIOR_ISO] / (float)PK;
        for (int t = 0; t < T4D_PRIORS_EDGE_TERMS; t++) add_seg(S, SEG_EDGE, kEdgeTerm[t], pr->n_edges[t], t, base[t], pr->weights[kEdgeTerm[t]]);
        for (int r = 0; r < T4D_PRIORS_REGION_TERMS; r++)
            add_seg(S, SEG_REGION, kRegionTerm[r], pr->n_region[r], r, base[T4D_PRIORS_EDGE_TERMS + r],
                    pr->weights[kRegionTerm[r]] / (3.f * (float)pr->n_region[r]));
    }
    return S;
}

struct Layout {
    size_t posR, posI, rotR, rotQ, rec, scale_g, partial, total;
};

Layout scratch_layout(const T4DPriors *pr)
{
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t PK = (size_t)pr->P * pr->K;
    const Segs a = make_segs(pr, 1), b = make_segs(pr, 0);
    const size_t blocks = (size_t)(a.blocks > b.blocks ? a.blocks : b.blocks);
    Layout L;
    size_t o = 0;
    L.posR = o; o = al(o + 16 * PK);
    L.posI = o; o = al(o + 16 * PK);
    L.rotR = o; o = al(o + 16 * PK);
    L.rotQ = o; o = al(o + 16 * PK);
    L.rec = o; o = al(o + 16 * (size_t)record_layout(pr, nullptr));
    L.scale_g = o; o = al(o + 16 * (size_t)pr->P);
    L.partial = o; o = al(o + sizeof(float) * kNbrTerms * blocks);
    L.total = o;
    return L;
}

bool valid(const T4DPriors *pr)
{
    if (!pr || pr->P < 1 || pr->K < 1 || (int64_t)pr->P * pr->K > 0x7fffffff / 4) return false;
    if (!pr->nbr || !pr->nbr_dist || !pr->rig_w || !pr->rot_w || !pr->iso_w || !pr->nbr_mask || !pr->nbr_num || !pr->init_scale ||
        !pr->nbr_t_off || !pr->nbr_t_idx || !pr->rec_off[0] || !pr->rec_off[1] || !pr->prev_inv_rot || !pr->prev_offset)
        return false;
    for (int t = 0; t < T4D_PRIORS_EDGE_TERMS; t++)
        if (pr->n_edges[t] < 0 || (pr->n_edges[t] > 0 && !pr->edges[t])) return false;
    for (int t = 0; t < 4; t++)
        if (pr->n_edges[2 + t] > 0 && !pr->cos_init[t]) return false;
    for (int r = 0; r < T4D_PRIORS_REGION_TERMS; r++)
        if (pr->n_region[r] < 0 || (pr->n_region[r] > 0 && !pr->region[r])) return false;
    const Segs a = make_segs(pr, 0);
    return a.n <= kMaxSegs;
}

}  // namespace

// train.py:328-368 (the regularisers of get_loss): see include/topo4d_raster.h
T4D_EXPORT int64_t t4d_priors_record_layout(const T4DPriors *pr, int64_t *base)
{
    if (!pr) return -1;
    return record_layout(pr, base);
}

T4D_EXPORT size_t t4d_priors_scratch_bytes(const T4DPriors *pr)
{
    if (!valid(pr)) {
        t4d_fail(T4D_ERR_ARG, "t4d_priors_scratch_bytes: bad topology");
        return 0;
    }
    return scratch_layout(pr).total;
}

T4D_EXPORT int t4d_priors_eval(const T4DPriors *pr, int32_t is_initial, const float *means3D, const float *unnorm_rotations,
                               const float *log_scales, float *d_means3D, float *d_unnorm_rotations, float *d_log_scales,
                               const float *upstream, uint32_t flags, float *losses, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!valid(pr) || !means3D || !unnorm_rotations || !log_scales || !d_means3D || !d_unnorm_rotations || !d_log_scales || !losses ||
        !scratch || (flags & ~(uint32_t)T4D_PRIORS_ACCUMULATE))
        return t4d_fail(T4D_ERR_ARG, "t4d_priors_eval: bad arguments");
    if (((uintptr_t)unnorm_rotations | (uintptr_t)pr->prev_inv_rot) & 15)
        return t4d_fail(T4D_ERR_ARG, "t4d_priors_eval: quaternion arrays must be 16-byte aligned");
    const Layout L = scratch_layout(pr);
    if (scratch_bytes < L.total) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_priors_eval: scratch too small");
    const Segs S = make_segs(pr, is_initial ? 1 : 0);
    char *base = (char *)scratch;
    Ptr p;
    p.x = means3D; p.q = unnorm_rotations; p.ls = log_scales;
    p.posR = (float4 *)(base + L.posR); p.posI = (float4 *)(base + L.posI);
    p.rotR = (float4 *)(base + L.rotR); p.rotQ = (float4 *)(base + L.rotQ);
    p.rec = (float4 *)(base + L.rec); p.scale_g = (float4 *)(base + L.scale_g);
    p.partial = (float *)(base + L.partial);
    hipStream_t stream = (hipStream_t)hip_stream;
    if (S.blocks > 0)
        hipLaunchKernelGGL(k_priors_elements, dim3((unsigned)S.blocks), dim3(kBlock), 0, stream, *pr, S, p, (int)(is_initial != 0));
    hipLaunchKernelGGL(k_priors_vertices, dim3((unsigned)((pr->P + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, *pr, S, p,
                       (int)(is_initial != 0), d_means3D, d_unnorm_rotations, d_log_scales, upstream,
                       (int)(flags & T4D_PRIORS_ACCUMULATE), losses);
    return t4d_launch_status("t4d_priors_eval");
}
