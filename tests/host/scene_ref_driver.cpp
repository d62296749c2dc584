// scene_ref_driver.cpp — TEST INFRASTRUCTURE.  Calls the reference's own compiled scene logic for tests/golden/make_scene_golden.py:
// Frustum::createFromMatrix / intersects (our_gl.cpp:212-280, linked from oracle/_ref/our_gl.o), AABB::transform and Plane::distance
// (geometry.h, included where the reference lies), Camera (camera.h) and, through oracle/_ref/model.o, Model::computeAABB.
// Nothing of the reference is copied here; the binary is built into a temporary directory and never kept.
//   scene_ref_driver <cases.txt> <results.txt>
// Every number travels as a C hex float (%a).  One case per line:
//   camera                                     -> view[16] proj[16] viewproj[16] sponza[16] head[16]   (main.cpp:506-513,585-594,610-623)
//   frustum   m[16]                            -> planes[24]
//   intersect planes[24] min[3] max[3]         -> 0 | 1          (the planes are set as given, not normalised again)
//   transform m[16] min[3] max[3]              -> min[3] max[3]
//   bounds    n stride v[n * stride]           -> min[3] max[3]  (Model::computeAABB; the position is the first 3 of each record)
#define private public          // Model::computeAABB and Model::vertices are private (model.h:98-130); access control does not change the layout
#include "model.h"
#undef private
#include "our_gl.h"
#include "camera.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

// the Importer that oracle/assimp_standin declares; no model file is ever read here
const aiScene* Assimp::Importer::ReadFile(const std::string&, unsigned int) { return nullptr; }
void Assimp::Importer::FreeScene() {}
const char* Assimp::Importer::GetErrorString() const { return "scene_ref_driver: no scene"; }

static double num(std::istream& in) { std::string t; in >> t; return std::strtod(t.c_str(), nullptr); }
static mat<4, 4> read_mat(std::istream& in) { mat<4, 4> m; for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m[r][c] = num(in); return m; }
static vec3 read_vec3(std::istream& in) { vec3 v; v.x = num(in); v.y = num(in); v.z = num(in); return v; }
static void put(std::ostream& out, double d) { char b[64]; std::snprintf(b, sizeof b, "%a ", d); out << b; }
static void put_mat(std::ostream& out, const mat<4, 4>& m) { for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) put(out, m[r][c]); }
static void put_vec3(std::ostream& out, const vec3& v) { put(out, v.x); put(out, v.y); put(out, v.z); }

int main(int argc, char** argv) {
    if (argc < 3) return 1;
    std::ifstream in(argv[1]);
    std::ofstream out(argv[2]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string what; ls >> what;
        if (what == "camera") {
            const int WIDTH = 1200, HEIGHT = 800;                       // main.cpp:26-27
            Camera camera;                                              // main.cpp:585-594
            camera.setEye(vec3{ -3.4019, 2.2001, 1.8026 });
            camera.setTarget(vec3{ 1.3555, 1.5116, -0.9686 });
            camera.setUp(vec3{ 0, 1, 0 });
            camera.setFOV(70.0);
            camera.setAspect((double)WIDTH / HEIGHT);
            camera.setClipping(0.05, 500.0);
            const mat<4, 4> view = camera.getViewMatrix(), proj = camera.getProjectionMatrix();
            // main.cpp:506-511: scale 0.014; translate (0, 1.6815, 0) * rotate about y by -112.82 degrees
            mat<4, 4> sponza = mat<4, 4>::identity(); sponza[0][0] = sponza[1][1] = sponza[2][2] = 0.014;
            mat<4, 4> tr = mat<4, 4>::identity(); tr[1][3] = 1.6815;
            const double a = -112.82 * M_PI / 180.0;
            mat<4, 4> ry = mat<4, 4>::identity(); ry[0][0] = cos(a); ry[0][2] = sin(a); ry[2][0] = -sin(a); ry[2][2] = cos(a);
            put_mat(out, view); put_mat(out, proj); put_mat(out, proj * view); put_mat(out, sponza); put_mat(out, tr * ry);
        } else if (what == "frustum") {
            const Frustum f = Frustum::createFromMatrix(read_mat(ls));
            for (int i = 0; i < 6; ++i) { put_vec3(out, f.planes[i].normal); put(out, f.planes[i].d); }
        } else if (what == "intersect") {
            Frustum f;
            for (int i = 0; i < 6; ++i) { f.planes[i].normal = read_vec3(ls); f.planes[i].d = num(ls); }
            const vec3 lo = read_vec3(ls), hi = read_vec3(ls);
            out << (f.intersects(AABB(lo, hi)) ? 1 : 0);
        } else if (what == "transform") {
            const mat<4, 4> m = read_mat(ls);
            const vec3 lo = read_vec3(ls), hi = read_vec3(ls);
            const AABB b = AABB(lo, hi).transform(m);
            put_vec3(out, b.min); put_vec3(out, b.max);
        } else if (what == "bounds") {
            const int n = (int)num(ls), stride = (int)num(ls);
            Model model("scene_ref_driver.obj");
            model.vertices.resize(n);
            for (int i = 0; i < n; ++i) {
                model.vertices[i].position = read_vec3(ls);
                for (int k = 3; k < stride; ++k) num(ls);
            }
            std::streambuf* keep = std::cout.rdbuf(nullptr);            // computeAABB prints the box (model.cpp:38-39)
            model.computeAABB();
            std::cout.rdbuf(keep);
            std::cout.clear();
            put_vec3(out, model.getLocalAABB().min); put_vec3(out, model.getLocalAABB().max);
        } else if (what.empty()) {
            continue;
        } else {
            std::fprintf(stderr, "scene_ref_driver: unknown case '%s'\n", what.c_str());
            return 2;
        }
        out << "\n";
    }
    return out ? 0 : 3;
}
