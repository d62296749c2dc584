"""HIP C++ sources of user shaders that restate the built-in kinds (include/trgl.h, "User shaders"), for the tests: a user kind
drawn with one of them must give the frame, depths and counters of the built-in kind it restates."""

FLAT = r"""
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) { return in.color; }
"""

# frag_gouraud and TGAColor::operator*(float) (tgaimage.h:55-62); the three intensities start at vary[OFFSET]
GOURAUD_TEMPLATE = r"""
#define OFFSET %d
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    const double* v = in.vary + OFFSET;
    double id = (v[0] * in.bar[0] + v[1] * in.bar[1]) + v[2] * in.bar[2];
    float intensity = (float)id;
    if (intensity < 0.f) intensity = 0.f;
    if (intensity > 1.f) intensity = 1.f;
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i) {
        float c = (float)(int)((in.color >> (8 * i)) & 0xff) * intensity;
        out |= (uint32_t)(uint8_t)c << (8 * i);
    }
    return out;
}
"""
GOURAUD = GOURAUD_TEMPLATE % 0
GOURAUD_PADDED = GOURAUD_TEMPLATE % 2      # K = 5: two doubles of padding ahead of the intensities

_COMMON = r"""
__device__ static double u_max(double a, double b) { return (a < b) ? b : a; }
__device__ static double u_min(double a, double b) { return (b < a) ? b : a; }
__device__ static double u_dot(const double* a, const double* b) { double s = 0; s += a[0] * b[0]; s += a[1] * b[1]; s += a[2] * b[2]; return s; }
__device__ static void u_normalized(const double* v, double* out) {
    double length = sqrt(u_dot(v, v));
    if (length == 0) { out[0] = v[0]; out[1] = v[1]; out[2] = v[2]; return; }
    out[0] = v[0] / length; out[1] = v[1] / length; out[2] = v[2] / length;
}
__device__ static void u_interp(const double* v0, const double* v1, const double* v2, const double* b, int n, double* out) {
    for (int i = 0; i < n; ++i) out[i] = (v0[i] * b[0] + v1[i] * b[1]) + v2[i] * b[2];
}
__device__ static double u_pow(double x, double y) { return (y == 1.0) ? x : pow(x, y); }
"""

# PhongShader::fragment (main.cpp:92-170), as the built-in PHONG kind computes it
PHONG = _COMMON + r"""
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    const trgl_uniforms& u = *in.u;
    const double* uvv = in.vary; const double* pos = in.vary + 6; const double* nrm = in.vary + 15;
    double position_eye[3], geometry_normal[3], uv[2];
    u_interp(pos, pos + 3, pos + 6, in.bar, 3, position_eye);
    u_interp(nrm, nrm + 3, nrm + 6, in.bar, 3, geometry_normal);
    u_interp(uvv, uvv + 2, uvv + 4, in.bar, 2, uv);
    const trgl_texel base = trgl_sample2D(in, u.tex_diffuse, uv);
    float specf = (float)(int)(trgl_sample2D(in, u.tex_specular, uv).bgra & 0xff) / 255.0f;     // (no map: white, 1.0f)
    double specular_power = u_max(1.0, (double)specf);
    int bsum = (int)(base.bgra & 0xff) + (int)((base.bgra >> 8) & 0xff) + (int)((base.bgra >> 16) & 0xff);
    double brightness = bsum / (3.0 * 255.0);
    bool is_eye_pixel = (brightness >= 0.85) && (specular_power <= 5.0);
    double nmv[3] = { 0, 0, 1 };
    if (u.tex_normal >= 0) {                        // (the tests upload every slot they name)
        const uint32_t c = trgl_sample2D(in, u.tex_normal, uv).bgra;
        double n[3];
        n[0] = (double)((c >> 16) & 0xff) / 255.0 * 2.0 - 1.0;
        n[1] = (double)((c >> 8) & 0xff) / 255.0 * 2.0 - 1.0;
        n[2] = (double)(c & 0xff) / 255.0 * 2.0 - 1.0;
        u_normalized(n, nmv);
    }
    double nme[3];
    for (int r = 0; r < 3; ++r) {
        const double* m = u.model_view + 4 * r;
        double sum = 0; sum += m[0] * nmv[0]; sum += m[1] * nmv[1]; sum += m[2] * nmv[2]; sum += m[3] * 0.0;
        nme[r] = sum;
    }
    double N[3];
    if (is_eye_pixel) { N[0] = geometry_normal[0]; N[1] = geometry_normal[1]; N[2] = geometry_normal[2]; }
    else {
        double s = u.normal_map_strength, mix[3];
        for (int i = 0; i < 3; ++i) mix[i] = geometry_normal[i] * (1.0 - s) + nme[i] * s;
        u_normalized(mix, N);
    }
    double negp[3], V[3];
    for (int i = 0; i < 3; ++i) negp[i] = position_eye[i] * -1.0;
    u_normalized(negp, V);
    const double* Lk = u.key_light_dir_eye;
    double key_diffuse = u_max(0.0, u_dot(N, Lk)) * 1.0;
    double k2 = 2.0 * u_dot(N, Lk), rr[3], R[3];
    for (int i = 0; i < 3; ++i) rr[i] = N[i] * k2 - Lk[i];
    u_normalized(rr, R);
    double rvd = u_max(0.0, u_dot(R, V));
    double key_specular = (rvd > 0.0 ? u_pow(rvd, specular_power) : 0.0) * 1.0;
    double fill_diffuse = u_max(0.0, u_dot(N, u.fill_light_dir_eye)) * 0.35;
    double rim_diffuse = u_max(0.0, u_dot(N, u.rim_light_dir_eye)) * 0.6;
    double total_diffuse = key_diffuse + fill_diffuse + rim_diffuse;
    double ambient = 0.10;
    uint32_t out = base.bgra & 0xff000000u;
    for (int ch = 0; ch < 3; ++ch) {
        double channel_value = (double)((base.bgra >> (8 * ch)) & 0xff);
        double final_value = channel_value * (ambient + total_diffuse) + 255.0 * (0.35 * key_specular);
        out |= (uint32_t)(unsigned char)u_min(255.0, final_value) << (8 * ch);
    }
    return out;
}
"""

# EyeShader::fragment (main.cpp:220-261), as the built-in EYE kind computes it
EYE = _COMMON + r"""
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    const trgl_uniforms& u = *in.u;
    const double* uvv = in.vary; const double* pos = in.vary + 6; const double* nrm = in.vary + 15;
    double position_eye[3], ni[3], N[3], uv[2];
    u_interp(pos, pos + 3, pos + 6, in.bar, 3, position_eye);
    u_interp(nrm, nrm + 3, nrm + 6, in.bar, 3, ni);
    u_normalized(ni, N);
    u_interp(uvv, uvv + 2, uvv + 4, in.bar, 2, uv);
    const trgl_texel base = trgl_sample2D(in, u.tex_diffuse, uv);
    double negp[3], V[3];
    for (int i = 0; i < 3; ++i) negp[i] = position_eye[i] * -1.0;
    u_normalized(negp, V);
    const double* Lk = u.key_light_dir_eye;
    double key_diffuse = u_max(0.0, u_dot(N, Lk)) * 1.0;
    double rim_diffuse = u_max(0.0, u_dot(N, u.rim_light_dir_eye)) * 0.6;
    double total_diffuse = key_diffuse + rim_diffuse;
    float specf = (float)(int)(trgl_sample2D(in, u.tex_specular, uv).bgra & 0xff) / 255.0f;     // (no map: white, 1.0f)
    double specular_power = u_max(1.0, (double)specf) * 8.0;
    double k2 = 2.0 * u_dot(N, Lk), rr[3], R[3];
    for (int i = 0; i < 3; ++i) rr[i] = N[i] * k2 - Lk[i];
    u_normalized(rr, R);
    double rvd = u_max(0.0, u_dot(R, V));
    double specular = (rvd > 0.0 ? u_pow(rvd, specular_power) : 0.0);
    uint32_t out = base.bgra & 0xff000000u;
    for (int ch = 0; ch < 3; ++ch) {
        double channel_value = (double)((base.bgra >> (8 * ch)) & 0xff);
        double final_value = channel_value * (0.1 + total_diffuse) + 255.0 * (1.5 * specular);
        out |= (uint32_t)(unsigned char)u_min(255.0, final_value) << (8 * ch);
    }
    return out;
}
"""
