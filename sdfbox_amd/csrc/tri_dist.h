// The squared distance from a point to a triangle, fp32, operation for operation the pinned rule of include/sdfhip.h
// (sdfhip_trimesh_build; -ffp-contract=off): what the mesh builder (trigen_kernels.h) and the nearest-surface search
// (distance_kernels.h) share, so that the two contracts read one definition.  __device__ __forceinline__ helpers only: any .hip may
// include it.  tests/trimesh_restatement.py restates it as _dist2.
#pragma once
#include <hip/hip_runtime.h>

namespace sdfhip {

__device__ __forceinline__ float tri_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// D of the rule; r = p - q and the region (0 face, 1 edge ab, 2 edge bc, 3 edge ca, 4 vertex a, 5 b, 6 c: the normal is at floats
// 9 + 3 * region of the record).  T: the nine position floats a, b, c -- nothing else is read.
__device__ __forceinline__ float tri_dist2(const float *T, float px, float py, float pz, float &rx, float &ry, float &rz, int &region)
{
    const float ax = T[0], ay = T[1], az = T[2], bx = T[3], by = T[4], bz = T[5], cx = T[6], cy = T[7], cz = T[8];
    const float abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float apx = px - ax, apy = py - ay, apz = pz - az;
    const float d1 = tri_dot(abx, aby, abz, apx, apy, apz), d2 = tri_dot(acx, acy, acz, apx, apy, apz);
    float qx, qy, qz;
    if (d1 <= 0.0f && d2 <= 0.0f) { qx = ax; qy = ay; qz = az; region = 4; }
    else {
        const float bpx = px - bx, bpy = py - by, bpz = pz - bz;
        const float d3 = tri_dot(abx, aby, abz, bpx, bpy, bpz), d4 = tri_dot(acx, acy, acz, bpx, bpy, bpz);
        if (d3 >= 0.0f && d4 <= d3) { qx = bx; qy = by; qz = bz; region = 5; }
        else {
            const float vc = d1 * d4 - d3 * d2;
            if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
                const float v = d1 / (d1 - d3);
                qx = ax + abx * v; qy = ay + aby * v; qz = az + abz * v; region = 1;
            } else {
                const float cpx = px - cx, cpy = py - cy, cpz = pz - cz;
                const float d5 = tri_dot(abx, aby, abz, cpx, cpy, cpz), d6 = tri_dot(acx, acy, acz, cpx, cpy, cpz);
                if (d6 >= 0.0f && d5 <= d6) { qx = cx; qy = cy; qz = cz; region = 6; }
                else {
                    const float vb = d5 * d2 - d1 * d6;
                    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
                        const float w = d2 / (d2 - d6);
                        qx = ax + acx * w; qy = ay + acy * w; qz = az + acz * w; region = 3;
                    } else {
                        const float va = d3 * d6 - d5 * d4;
                        const float e0 = d4 - d3, e1 = d5 - d6;
                        if (va <= 0.0f && e0 >= 0.0f && e1 >= 0.0f) {
                            const float w = e0 / (e0 + e1);
                            qx = bx + (cx - bx) * w; qy = by + (cy - by) * w; qz = bz + (cz - bz) * w; region = 2;
                        } else {
                            const float den = 1.0f / ((va + vb) + vc);
                            const float v = vb * den, w = vc * den;
                            qx = (ax + abx * v) + acx * w; qy = (ay + aby * v) + acy * w; qz = (az + abz * v) + acz * w; region = 0;
                        }
                    }
                }
            }
        }
    }
    rx = px - qx; ry = py - qy; rz = pz - qz;
    return tri_dot(rx, ry, rz, rx, ry, rz);
}

}  // namespace sdfhip
