// Shared primitives of the articulated-body physics for gfx950 (the solver itself: lg_physics_pair.h).
//
// Replaces gym.simulate() (reference call site legged_gym/envs/base/legged_robot.py:92-96).  The
// algorithm is the build's own specification (oracle/lgo_physics.cpp restates it scalar, generic
// tree): Featherstone ABA in base-frame coordinates about the base origin, exact 3x3 contact-space
// inverse inertia per sphere contact from test impulses, projected-Jacobi sweeps over contacts and
// joint-limit constraints, one tree impulse propagation per sweep, semi-implicit Euler.
//
// This header holds what the solver builds on: the joint and base rotations, the launch constants
// it keeps in registers (PhysCfg), the heightfield lookup, and the layout of the LDS records it
// shares with the control loop (contact slots, links).
#pragma once
#include "lg_device.h"

__device__ __forceinline__ M3 rodrigues(V3 a, float th) {
    const float s = __sinf(th), c = __cosf(th);      // |th| is a joint angle: the fast forms are accurate to ~1e-6
    float t = 1.0f - c;
    M3 R = {{{c + t * a.x * a.x, t * a.x * a.y - s * a.z, t * a.x * a.z + s * a.y},
             {t * a.x * a.y + s * a.z, c + t * a.y * a.y, t * a.y * a.z - s * a.x},
             {t * a.x * a.z - s * a.y, t * a.y * a.z + s * a.x, c + t * a.z * a.z}}};
    return R;
}
__device__ __forceinline__ M3 quat_to_mat(const float *q) {
    float x = q[0], y = q[1], z = q[2], w = q[3];
    M3 R = {{{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
             {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
             {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}}};
    return R;
}

// The scalars of DevParams the physics reads in every substep, copied into registers ONCE per launch (phys_cfg): read through P they are
// scalar loads the compiler must repeat after every workgroup barrier of the control loop (29 s_load per substep pass, each cluster a
// ~150-cycle wait for the lone physics wave).  Field names follow lg_cfg, so the physics reads `c.<name>` either way.
struct PhysCfg {
    float gravity[3];
    float max_depenetration_velocity, contact_erp, ground_restitution, ground_friction, contact_offset, bounce_threshold;
    float max_linear_velocity, max_angular_velocity, armature, rest_offset;
    float border_size, hf_hscale, hf_vscale, hf_inv_hscale;
    int hf_rows, hf_cols, terrain_type, solver_iterations, material_rand;
    int n_leg_slots, n_base_spheres;
    unsigned long long slot_link_pk;
    const int16_t *height_samples;
    float base_mass, base_com[3], base_inertia[9];
};
__device__ __forceinline__ PhysCfg phys_cfg(const DevParams *__restrict__ P) {
    const lg_cfg &c = P->cfg;
    PhysCfg k;
    for (int i = 0; i < 3; ++i) k.gravity[i] = c.gravity[i];
    k.max_depenetration_velocity = c.max_depenetration_velocity; k.contact_erp = c.contact_erp;
    k.ground_restitution = c.ground_restitution; k.ground_friction = c.ground_friction;
    k.contact_offset = c.contact_offset; k.bounce_threshold = c.bounce_threshold;
    k.max_linear_velocity = c.max_linear_velocity; k.max_angular_velocity = c.max_angular_velocity;
    k.armature = c.armature; k.rest_offset = c.rest_offset;
    k.border_size = c.border_size; k.hf_hscale = c.hf_hscale; k.hf_vscale = c.hf_vscale;
    k.hf_inv_hscale = 1.0f / c.hf_hscale;
    k.hf_rows = c.hf_rows; k.hf_cols = c.hf_cols; k.terrain_type = c.terrain_type;
    k.solver_iterations = c.solver_iterations; k.material_rand = c.material_rand;
    k.n_leg_slots = P->n_leg_slots; k.n_base_spheres = P->n_base_spheres; k.slot_link_pk = P->slot_link_pk;
    k.height_samples = P->height_samples;
    k.base_mass = P->model.mass[0];
    for (int i = 0; i < 3; ++i) k.base_com[i] = P->model.com[0][i];
    for (int i = 0; i < 9; ++i) k.base_inertia[i] = P->model.inertia[0][i];
    return k;
}

struct Ground { float h; V3 n; };
// The heightfield lookup in two halves, so that a caller with several points can have all their samples in flight before it needs the
// first (lg_physics_pair.h: eight collision spheres per lane, eight round trips to the L2 one after the other otherwise).
struct GroundTap { int16_t s00, s01, s10, s11; float tx, ty; };
// The four divisions by the grid pitch per point are products with its reciprocal (32 IEEE divisions per lane and substep otherwise, a
// third of the detection's instructions; the oracle defines the lookup the same way).
__device__ __forceinline__ GroundTap ground_fetch(const PhysCfg &c, const int16_t *__restrict__ height_samples, float x, float y) {
    if (c.terrain_type == 0) return {0, 0, 0, 0, 0.f, 0.f};
    float gx = (x + c.border_size) * c.hf_inv_hscale, gy = (y + c.border_size) * c.hf_inv_hscale;
    gx = fminf(fmaxf(gx, 0.0f), (float)(c.hf_rows - 1) - 1e-3f);
    gy = fminf(fmaxf(gy, 0.0f), (float)(c.hf_cols - 1) - 1e-3f);
    int ix = (int)gx, iy = (int)gy;
    const int16_t *hs = height_samples + (size_t)ix * c.hf_cols + iy;
    return {hs[0], hs[1], hs[c.hf_cols], hs[c.hf_cols + 1], gx - ix, gy - iy};
}
__device__ __forceinline__ Ground ground_finish(const PhysCfg &c, const GroundTap &t) {
    if (c.terrain_type == 0) return {0.0f, {0.0f, 0.0f, 1.0f}};
    const float tx = t.tx, ty = t.ty;
    float h00 = (float)t.s00 * c.hf_vscale, h01 = (float)t.s01 * c.hf_vscale;
    float h10 = (float)t.s10 * c.hf_vscale, h11 = (float)t.s11 * c.hf_vscale;
    float h = (1 - tx) * (1 - ty) * h00 + tx * (1 - ty) * h10 + (1 - tx) * ty * h01 + tx * ty * h11;
    float dhdx = ((1 - ty) * (h10 - h00) + ty * (h11 - h01)) * c.hf_inv_hscale;
    float dhdy = ((1 - tx) * (h01 - h00) + tx * (h11 - h10)) * c.hf_inv_hscale;
    float inv = rsqrtf(dhdx * dhdx + dhdy * dhdy + 1.0f);
    return {h, {-dhdx * inv, -dhdy * inv, inv}};
}

#define LG_CT_NF 19      // floats per contact-slot record: Pc 3 (sphere centre before detection), n 3, W 6, target, impulses 3, first tangent 3 
#define LG_LK_NF 24      // floats per link and pair of the link records: shared R 9, p 3 (LG_LKP_NF) + each lane's half of vel, c (2 x LG_LKH_NF)
__device__ __forceinline__ void tangents(V3 n, V3 &t1, V3 &t2) {
    V3 ref = fabsf(n.x) < 0.9f ? V3{1.f, 0.f, 0.f} : V3{0.f, 1.f, 0.f};
    V3 t = cross(n, ref);
    t1 = rsqrtf(dot(t, t)) * t;
    t2 = cross(n, t1);
}
