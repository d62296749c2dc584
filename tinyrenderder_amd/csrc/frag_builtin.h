// frag_builtin.h — the fragment bodies of the built-in shader kinds (main.cpp's PhongShader and EyeShader, GOURAUD, CHECKER) and their
// vector helpers, in the reference's operation order: what k_raster and k_shade (kernels_raster.hip) call per fragment.
#pragma once
#include "shade_common.h"

namespace trgl_shade {

__device__ __forceinline__ double dot3(const double* a, const double* b) {
    double sum = 0; sum += a[0] * b[0]; sum += a[1] * b[1]; sum += a[2] * b[2]; return sum;   // geometry.h:122-127
}
__device__ __forceinline__ void normalized3(const double* v, double* out) {                   // geometry.h:136-140
    double length = sqrt(dot3(v, v));
    if (length == 0) { out[0] = v[0]; out[1] = v[1]; out[2] = v[2]; return; }
    out[0] = v[0] / length; out[1] = v[1] / length; out[2] = v[2] / length;
}

__device__ __forceinline__ void interp(const double* v0, const double* v1, const double* v2, const double* b, int n, double* out) {
    for (int i = 0; i < n; ++i) out[i] = (v0[i] * b[0] + v1[i] * b[1]) + v2[i] * b[2];       // main.cpp:94-104
}
__device__ __forceinline__ double spec_pow(double x, double y) {
    // std::pow(x, 1.0) == x exactly; PhongShader's exponent is always 1.0
    return (y == 1.0) ? x : pow(x, y);
}

// PhongShader::fragment — main.cpp:92-170
template <class UN, class TX>
__device__ __forceinline__ Color frag_phong(const UN& u, TX tx, const double* vary, const double* b) {
    const double* uvv = vary; const double* pos = vary + 6; const double* nrm = vary + 15;
    double position_eye[3], geometry_normal[3], uv[2];
    interp(pos, pos + 3, pos + 6, b, 3, position_eye);
    interp(nrm, nrm + 3, nrm + 6, b, 3, geometry_normal);
    interp(uvv, uvv + 2, uvv + 4, b, 2, uv);

    // the three maps are independent: issue all texel loads first, consume afterwards (the slots are per draw,
    // so these branches are wave-uniform)
    const TX td = tex_slot(tx, u.tex_diffuse);
    const TX ts = tex_slot(tx, u.tex_specular);
    const TX tn = tex_slot(tx, u.tex_normal);
    uint32_t raw_d = 0, raw_s = 0, raw_n = 0;
    if (td) raw_d = tex_fetch_raw(td, uv);
    if (ts) raw_s = tex_fetch_raw(ts, uv);
    if (tn) raw_n = tex_fetch_raw(tn, uv);
    Color base = td ? Color{ raw_d & tex_mask(td), td->bpp } : Color{ 0xffffffffu, 4 };       // model.cpp:415-426
    float specf = ts ? (float)(int)(raw_s & 0xff) / 255.0f : 1.0f;                            // model.cpp:447-459
    double specular_power = dmax(1.0, (double)specf);

    int bsum = (int)(base.bgra & 0xff) + (int)((base.bgra >> 8) & 0xff) + (int)((base.bgra >> 16) & 0xff);
    double brightness = bsum / (3.0 * 255.0);
    bool is_eye_pixel = (brightness >= 0.85) && (specular_power <= 5.0);

    double nmv[3] = { 0, 0, 1 };                                                              // model.cpp:428-445
    if (tn) {
        const uint32_t c = raw_n & tex_mask(tn);
        double n[3];
        n[0] = (double)((c >> 16) & 0xff) / 255.0 * 2.0 - 1.0;
        n[1] = (double)((c >> 8) & 0xff) / 255.0 * 2.0 - 1.0;
        n[2] = (double)(c & 0xff) / 255.0 * 2.0 - 1.0;
        normalized3(n, nmv);
    }
    double nme[3];                                                                            // main.cpp:116-119
    for (int r = 0; r < 3; ++r) {
        const auto* m = u.model_view + 4 * r;
        double sum = 0; sum += m[0] * nmv[0]; sum += m[1] * nmv[1]; sum += m[2] * nmv[2]; sum += m[3] * 0.0;
        nme[r] = sum;
    }
    double N[3];
    if (is_eye_pixel) { N[0] = geometry_normal[0]; N[1] = geometry_normal[1]; N[2] = geometry_normal[2]; }
    else {
        double s = u.normal_map_strength, mix[3];
        for (int i = 0; i < 3; ++i) mix[i] = geometry_normal[i] * (1.0 - s) + nme[i] * s;
        normalized3(mix, N);
    }
    double negp[3], V[3];
    for (int i = 0; i < 3; ++i) negp[i] = position_eye[i] * -1.0;
    normalized3(negp, V);

    const double Lk[3] = { u.key_light_dir_eye[0], u.key_light_dir_eye[1], u.key_light_dir_eye[2] };
    double key_diffuse = dmax(0.0, dot3(N, Lk)) * 1.0;
    double k2 = 2.0 * dot3(N, Lk), rr[3], R[3];
    for (int i = 0; i < 3; ++i) rr[i] = N[i] * k2 - Lk[i];
    normalized3(rr, R);
    double rvd = dmax(0.0, dot3(R, V));
    double key_specular = (rvd > 0.0 ? spec_pow(rvd, specular_power) : 0.0) * 1.0;
    const double Lf[3] = { u.fill_light_dir_eye[0], u.fill_light_dir_eye[1], u.fill_light_dir_eye[2] };
    double fill_diffuse = dmax(0.0, dot3(N, Lf)) * 0.35;
    const double Lr[3] = { u.rim_light_dir_eye[0], u.rim_light_dir_eye[1], u.rim_light_dir_eye[2] };
    double rim_diffuse = dmax(0.0, dot3(N, Lr)) * 0.6;
    double total_diffuse = key_diffuse + fill_diffuse + rim_diffuse;
    double total_specular = key_specular;
    double ambient = 0.10;

    uint32_t out = base.bgra & 0xff000000u;
    for (int ch = 0; ch < 3; ++ch) {
        double channel_value = (double)((base.bgra >> (8 * ch)) & 0xff);
        double final_value = channel_value * (ambient + total_diffuse) + 255.0 * (0.35 * total_specular);
        out |= (uint32_t)(unsigned char)dmin(255.0, final_value) << (8 * ch);
    }
    return Color{ out, base.bytespp };
}

// EyeShader::fragment — main.cpp:220-261
template <class UN, class TX>
__device__ __forceinline__ Color frag_eye(const UN& u, TX tx, const double* vary, const double* b) {
    const double* uvv = vary; const double* pos = vary + 6; const double* nrm = vary + 15;
    double position_eye[3], ni[3], N[3], uv[2];
    interp(pos, pos + 3, pos + 6, b, 3, position_eye);
    interp(nrm, nrm + 3, nrm + 6, b, 3, ni);
    normalized3(ni, N);
    interp(uvv, uvv + 2, uvv + 4, b, 2, uv);

    const TX td = tex_slot(tx, u.tex_diffuse);
    const TX ts = tex_slot(tx, u.tex_specular);
    uint32_t raw_d = 0, raw_s = 0;
    if (td) raw_d = tex_fetch_raw(td, uv);
    if (ts) raw_s = tex_fetch_raw(ts, uv);
    Color base = td ? Color{ raw_d & tex_mask(td), td->bpp } : Color{ 0xffffffffu, 4 };
    double negp[3], V[3];
    for (int i = 0; i < 3; ++i) negp[i] = position_eye[i] * -1.0;
    normalized3(negp, V);

    const double Lk[3] = { u.key_light_dir_eye[0], u.key_light_dir_eye[1], u.key_light_dir_eye[2] };
    double key_diffuse = dmax(0.0, dot3(N, Lk)) * 1.0;
    const double Lr[3] = { u.rim_light_dir_eye[0], u.rim_light_dir_eye[1], u.rim_light_dir_eye[2] };
    double rim_diffuse = dmax(0.0, dot3(N, Lr)) * 0.6;
    double total_diffuse = key_diffuse + rim_diffuse;

    float specf = ts ? (float)(int)(raw_s & 0xff) / 255.0f : 1.0f;
    double specular_power = dmax(1.0, (double)specf) * 8.0;
    double k2 = 2.0 * dot3(N, Lk), rr[3], R[3];
    for (int i = 0; i < 3; ++i) rr[i] = N[i] * k2 - Lk[i];
    normalized3(rr, R);
    double rvd = dmax(0.0, dot3(R, V));
    double specular = (rvd > 0.0 ? spec_pow(rvd, specular_power) : 0.0);

    uint32_t out = base.bgra & 0xff000000u;
    for (int ch = 0; ch < 3; ++ch) {
        double channel_value = (double)((base.bgra >> (8 * ch)) & 0xff);
        double final_value = channel_value * (0.1 + total_diffuse) + 255.0 * (1.5 * specular);
        out |= (uint32_t)(unsigned char)dmin(255.0, final_value) << (8 * ch);
    }
    return Color{ out, base.bytespp };
}

// GOURAUD: base * (float)(i0*b0 + i1*b1 + i2*b2), TGAColor::operator*(float) tgaimage.h:55-62
__device__ __forceinline__ uint32_t frag_gouraud(uint32_t base, const double* vary, const double* b) {
    double id = (vary[0] * b[0] + vary[1] * b[1]) + vary[2] * b[2];
    float intensity = (float)id;
    if (intensity < 0.f) intensity = 0.f;
    if (intensity > 1.f) intensity = 1.f;
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i) {
        float c = (float)(int)((base >> (8 * i)) & 0xff) * intensity;
        out |= (uint32_t)(uint8_t)c << (8 * i);
    }
    return out;
}


// CHECKER: a FLAT colour that discards on a predicate of the perspective-correct barycentrics - the device kind that exercises
// `if (discard) continue;` (our_gl.cpp:187-188): cell parities of bar[0] and bar[1] on a cells x cells grid differ -> discard.
__device__ __forceinline__ bool frag_checker_discards(int cells, const double* b) {
    const int a = x86_cvttsd2si(b[0] * (double)cells), c = x86_cvttsd2si(b[1] * (double)cells);
    return ((a ^ c) & 1) != 0;
}

}  // namespace trgl_shade
