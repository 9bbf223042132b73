// An assembly of placed instances, consumed without baking (gfx950): k_instances_sample (value, winner and gradient at n points),
// k_instances_march (the primary march for n rays, or for n pixels of a camera block) and k_instances_render (a frame).  Host
// side, C ABI: instances.hip.
//
// Replaces: nothing in the reference's code -- its shader marches ONE immutable tree.  Here find + interpol_world of Compute.hlsl
// become the fold of sdfhip_scene_compose over the call's instance table, evaluated at the marched point itself; no tree is built.
//
// The rule is the contract of include/sdfhip.h (sdfhip_instances_*) and DESIGN.md section 8 (N17): fp32, each operation rounded on
// its own, in the order written (-ffp-contract=off; the shader's fused operations are explicit fmaf, as in raymarch_device.h);
// tests/instances_restatement.py restates it with numpy on compose_restatement.value.
//   u_k(p)    place_value (place_kernels.h) of instance k's source under instance k's map, by the instance's cursor form
//             (compose_instance_value): every look-up starts at the root, no cursor is carried, so F depends on the point alone
//   F(p)      v = u_0; then in list order UNION fminf(v, u_k), INTERSECT fmaxf(v, u_k), SUBTRACT fmaxf(v, -u_k); of two zeros of
//             opposite sign fminf is -0 and fmaxf +0 (the header pins it: v_min_f32 / v_max_f32 order -0 below +0, and the MI355X
//             returns +0 for fmaxf(+0, -0), tests/test_gpu_instances_zoo.py's "signtie")
//   w(p)      w = 0; UNION: w = k iff u_k < v before the fold; INTERSECT: iff u_k > v; SUBTRACT: iff -u_k > v (ties keep the earlier)
//   G(p)      (F(p + (h,0,0)) - F(p - (h,0,0)), F(p + (0,h,0)) - F(p - (0,h,0)), F(p + (0,0,h)) - F(p - (0,0,h))), h = normal_step;
//             the offsets are added as vectors: the other two coordinates are p_a + 0.0f and p_a - 0.0f
//
// The exact skip.  place_value computes e = sqrtf((ex*ex + ey*ey) + ez*ez), the distance from the inverse-mapped point to the
// source's cube, before it looks anything up, and returns (D + e) * s with D the source's sampled distance at the clamped point.
// D >= -0.5625 for every tree an upload accepts, because of how D is decoded (raymarch_device.h, sdf_bytes.h):
//   * a texel is unorm8(byte) = byte / 255 in [0, 1] for every byte 0..255 -- the upload refuses links, never bytes;
//   * lerp(a, b, t) = fmaf(t, b - a, a) with a, b in [lo, hi] and t in [0, 1] (sat() makes it so, NaN -> 0): the exact t (b - a) + a
//     lies in [lo, hi]; b - a is rounded once (error <= 2^-24 for |b - a| <= 1 + 2^-20) and the fmaf once more, so the result lies
//     in [lo - 2^-22, hi + 2^-22]; the trilinear blend is three such levels: L >= -2^-20;
//   * D = (L - 0.25f) * scale * 2.0f, and scale = 2^-level <= 1: find_fresh starts at the root, whose box is the unit cube and
//     holds the clamped point, so no cursor ever ascends and `scale` is only ever halved from 1 (a grid cell carries its level the
//     same way; a flat cell stores the same expression on eight equal texels, flat_cell_distance_bits); so
//     D >= (-2^-20 - 0.25) * 2 > -0.5001.
// -0.5625 = -0.5 - 2^-4 leaves that room sixty thousand times over.  The bound b_k = (-0.5625f + e) * s has the operation shape of
// (D + e) * s: fl(-0.5625 + e) <= fl(D + e) and the multiplication by s > 0 keeps the order (rounding is monotone), so b_k <= u_k
// with no error term.  For k >= 1 a UNION instance is skipped iff b_k > v (then u_k > v: fminf(v, u_k) = v, and u_k < v is
// false); a SUBTRACT instance iff -b_k < v (then -u_k < v: fmaxf(v, -u_k) = v, and -u_k > v is false); an INTERSECT instance and
// instance 0 never.  A NaN on either side makes the comparison false: evaluated.  So the skip changes no bit of any output
// (tests/test_gpu_instances.py runs every case with and without it).  e is computed here by place_value's own lines, so the
// compiler may share them with the look-up that follows.
//
// Shape.  One lane per point, ray or pixel; pixels in 8 x 8 tiles per wave.  The instance loop is wave-uniform -- the list, its
// bound, the table index and each instance's op and form are the same for every lane -- and the table is read through a uniform
// index; lanes diverge on the skip only.  G is a loop over its six taps round ONE inlined F, not six copies of it.
#pragma once
#include "compose_instance.h"   // ComposeInstance, compose_instance_value, place_lower_bound; place_kernels.h, query_kernels.h, raymarch_device.h

namespace sdfhip {

constexpr int INSTANCES_THREADS = 256;

// the call's assembly as a kernel reads it
struct PartField {
    const ComposeInstance *table;
    uint32_t n;             // >= 1
    uint32_t skip;          // 0: every instance is looked up at every point (SDFHIP_INSTANCES_NO_SKIP)
    float h;                // normal_step
};

// F(p), and w(p) beside it
__device__ __forceinline__ float part_field(const PartField &A, float px, float py, float pz, uint32_t &w)
{
    float v = 0.0f;
    w = 0u;
    for (uint32_t k = 0; k < A.n; k++) {
        const ComposeInstance &I = A.table[k];
        const int32_t op = I.op;
        if (A.skip && k != 0 && op != COMPOSE_INTERSECT) {
            const float b = place_lower_bound(I.M, px, py, pz);
            if (op == COMPOSE_UNION ? b > v : -b < v) continue;
        }
        const float u = compose_instance_value(I, px, py, pz);
        if (k == 0) { v = u; continue; }                      // (the host has made sure that instance 0 is a union)
        switch (op) {
        case COMPOSE_UNION: if (u < v) w = k; v = fminf(v, u); break;
        case COMPOSE_INTERSECT: if (u > v) w = k; v = fmaxf(v, u); break;
        default: { const float nu = -u; if (nu > v) w = k; v = fmaxf(v, nu); } break;
        }
    }
    return v;
}

// G(p): tap 2a is p + h e_a, tap 2a + 1 is p - h e_a
__device__ __forceinline__ void part_gradient(const PartField &A, float px, float py, float pz, float &gx, float &gy, float &gz)
{
    gx = gy = gz = 0.0f;
    float plus = 0.0f;
#pragma nounroll
    for (int tap = 0; tap < 6; tap++) {
        const int axis = tap >> 1;
        const bool minus = (tap & 1) != 0;
        const float ox = axis == 0 ? A.h : 0.0f, oy = axis == 1 ? A.h : 0.0f, oz = axis == 2 ? A.h : 0.0f;
        const float qx = minus ? px - ox : px + ox, qy = minus ? py - oy : py + oy, qz = minus ? pz - oz : pz + oz;
        uint32_t w;
        const float f = part_field(A, qx, qy, qz, w);
        if (!minus) plus = f;
        else {
            const float d = plus - f;
            if (axis == 0) gx = d; else if (axis == 1) gy = d; else gz = d;
        }
    }
}

// sample: F, w and G at point i.  A non-finite coordinate: SDFHIP_QUERY_INVALID and zeros, nothing looked up.
// xyz: n x 3 floats, packed; out: n records of two uint4 {value, instance, status, 0 | gradient, 0}
__global__ __launch_bounds__(INSTANCES_THREADS) void k_instances_sample(PartField A, const float *__restrict__ xyz, uint32_t n, uint4 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * INSTANCES_THREADS + threadIdx.x;
    if (i >= n) return;
    const float px = xyz[3 * (size_t)i], py = xyz[3 * (size_t)i + 1], pz = xyz[3 * (size_t)i + 2];
    uint4 a = make_uint4(0u, 0u, (uint32_t)QUERY_INVALID, 0u), b = make_uint4(0u, 0u, 0u, 0u);
    if (finite3(px, py, pz)) {
        uint32_t w;
        const float v = part_field(A, px, py, pz, w);
        float gx, gy, gz;
        part_gradient(A, px, py, pz, gx, gy, gz);
        a = make_uint4(__float_as_uint(v), w, (uint32_t)QUERY_HIT, 0u);
        b = make_uint4(__float_as_uint(gx), __float_as_uint(gy), __float_as_uint(gz), 0u);
    }
    record_store<true>(out + 2 * (size_t)i, a);
    record_store<true>(out + 2 * (size_t)i + 1, b);
}

// march: the loop of k_query_march (Compute.hlsl:194-203) with find + interpol_world replaced by F:
//     prox = 1; i = 0; t = 0; w = 0
//     while ((prox > margin2 || prox < 0) && i < max_steps) {
//         if (dot(pos, pos) > limit) -> ESCAPED
//         prox = F(pos); w = w(pos); pos = fma(dir, prox, pos); t = t + prox; i++ }
//     -> HIT if !(prox > margin2 || prox < 0), else EXHAUSTED
// PICK = false: `in` = n rays {origin, pad, dir, pad}; PICK = true: `in` = n pixels {x, y}, the ray is ray() of raymarch_device.h.
// A non-finite origin or direction, or a direction of all zeros: SDFHIP_QUERY_INVALID and zeros, nothing looked up.
// out: n records of three uint4 {position, t | normal, prox | status, steps, instance, 0}; normal = G(position) * (1 / sqrtf(dot(G, G)))
template <bool PICK>
__global__ __launch_bounds__(INSTANCES_THREADS) void k_instances_march(PartField A, const void *__restrict__ in, uint32_t n, FrameInfo I,
                                                                       uint32_t max_steps, uint4 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * INSTANCES_THREADS + threadIdx.x;
    if (i >= n) return;
    float px, py, pz, dx, dy, dz;
    if (PICK) {
        const uint2 xy = static_cast<const uint2 *>(in)[i];
        px = I.posx; py = I.posy; pz = I.posz;
        ray(I, xy.x, xy.y, dx, dy, dz);
    } else {
        const float4 o = static_cast<const float4 *>(in)[2 * (size_t)i], d = static_cast<const float4 *>(in)[2 * (size_t)i + 1];
        px = o.x; py = o.y; pz = o.z; dx = d.x; dy = d.y; dz = d.z;
    }
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a, e = make_uint4((uint32_t)QUERY_INVALID, 0u, 0u, 0u);
    if (finite3(px, py, pz) && finite3(dx, dy, dz) && !(dx == 0.0f && dy == 0.0f && dz == 0.0f)) {
        float prox = 1.0f, t = 0.0f;
        uint32_t steps = 0u, w = 0u;
        bool escaped = false;
        while ((prox > I.margin2 || prox < 0.0f) && steps < max_steps) {
            if (dot3(px, py, pz, px, py, pz) > I.limit) { escaped = true; break; }
            prox = part_field(A, px, py, pz, w);
            px = __builtin_fmaf(dx, prox, px); py = __builtin_fmaf(dy, prox, py); pz = __builtin_fmaf(dz, prox, pz);
            t = t + prox;
            steps++;
        }
        const uint32_t status = escaped ? (uint32_t)QUERY_ESCAPED : (prox > I.margin2 || prox < 0.0f) ? (uint32_t)QUERY_EXHAUSTED : (uint32_t)QUERY_HIT;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (!escaped) {
            float gx, gy, gz;
            part_gradient(A, px, py, pz, gx, gy, gz);
            const float rg = 1.0f / sqrtf(dot3(gx, gy, gz, gx, gy, gz));
            nx = gx * rg; ny = gy * rg; nz = gz * rg;
        }
        a = make_uint4(__float_as_uint(px), __float_as_uint(py), __float_as_uint(pz), __float_as_uint(t));
        b = make_uint4(__float_as_uint(nx), __float_as_uint(ny), __float_as_uint(nz), __float_as_uint(prox));
        e = make_uint4(status, steps, w, 0u);
    }
    record_store<true>(out + 3 * (size_t)i, a);
    record_store<true>(out + 3 * (size_t)i + 1, b);
    record_store<true>(out + 3 * (size_t)i + 2, e);
}

// render: main() of Compute.hlsl:180-231 (oracle/sdf_oracle.c o_pixel) for pixel (x, y), line for line, with find + interpol_world
// replaced by F and gradient() by G -- at the shading point and inside the shadow loop's prox < margin test -- and 100 by max_steps.
// A wave is an 8 x 8 tile of the frame, a workgroup four consecutive tiles in row-major tile order.  out: width x height float4,
// tightly packed, row 0 at the top; alpha = the march's steps.
__global__ __launch_bounds__(INSTANCES_THREADS) void k_instances_render(PartField A, FrameInfo I, uint32_t max_steps, uint32_t width, uint32_t height,
                                                                        uint32_t tiles_x, uint32_t n_tiles, uint4 *__restrict__ out)
{
    const uint32_t tile = blockIdx.x * (INSTANCES_THREADS / 64) + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = (tile % tiles_x) * 8u + (lane & 7u), y = (tile / tiles_x) * 8u + (lane >> 3);
    if (x >= width || y >= height) return;

    float px = I.posx, py = I.posy, pz = I.posz, dx, dy, dz;
    ray(I, x, y, dx, dy, dz);
    const float margin = I.margin;
    float prox = 1.0f;
    uint32_t i = 0u, j = 0u, w;
    bool sky = false;
    while ((prox > I.margin2 || prox < 0.0f) && i < max_steps) {
        if (dot3(px, py, pz, px, py, pz) > I.limit) { sky = true; break; }
        prox = part_field(A, px, py, pz, w);
        px = __builtin_fmaf(dx, prox, px); py = __builtin_fmaf(dy, prox, py); pz = __builtin_fmaf(dz, prox, pz);
        i++;
    }
    float r = 0.0f, g = 0.0f, bl = 0.0f;
    if (sky) { r = 0.005f; g = 0.01f; bl = 0.2f; }
    else {
        // dir = normalize(light - pos); pos += dir * margin
        float lx = I.lightx - px, ly = I.lighty - py, lz = I.lightz - pz;
        const float rl = 1.0f / sqrtf(dot3(lx, ly, lz, lx, ly, lz));
        dx = lx * rl; dy = ly * rl; dz = lz * rl;
        px = __builtin_fmaf(dx, margin, px); py = __builtin_fmaf(dy, margin, py); pz = __builtin_fmaf(dz, margin, pz);
        // angle = dot(dir, normalize(G(pos)))
        float gx, gy, gz;
        part_gradient(A, px, py, pz, gx, gy, gz);
        const float rg = 1.0f / sqrtf(dot3(gx, gy, gz, gx, gy, gz));
        const float angle = dot3(dx, dy, dz, gx * rg, gy * rg, gz * rg);
        if (!(angle < 0.0f)) {
            lx = I.lightx - px; ly = I.lighty - py; lz = I.lightz - pz;
            const float dist = sqrtf(dot3(lx, ly, lz, lx, ly, lz)) / 2.0f;
            bool lit = false;
            for (; j < 40u && prox > -margin; j++) {
                if (prox > dist || (px < 0.0f || py < 0.0f || pz < 0.0f) || (px > 1.0f || py > 1.0f || pz > 1.0f)) { lit = true; break; }
                if (prox < margin) {
                    part_gradient(A, px, py, pz, gx, gy, gz);
                    if (dot3(gx, gy, gz, dx, dy, dz) < 0.0f) break;
                }
                prox = part_field(A, px, py, pz, w);
                const float step = prox + margin;
                px = __builtin_fmaf(dx, step, px); py = __builtin_fmaf(dy, step, py); pz = __builtin_fmaf(dz, step, pz);
            }
            if (lit) r = g = bl = angle / (dist * dist) * I.k_strength;
        }
    }
    record_store<true>(out + (size_t)y * width + x, make_uint4(__float_as_uint(r), __float_as_uint(g), __float_as_uint(bl), __float_as_uint((float)(i + j))));
}

}  // namespace sdfhip
