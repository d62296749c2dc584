// mesh_attr_ref_driver.cpp — TEST INFRASTRUCTURE.  Calls the reference's own compiled Model::generateNormalsIfNeeded and
// Model::computeTangentsIfNeeded (model.cpp:269-388, linked from oracle/_ref/model.o) for tests/golden/make_mesh_attr_golden.py.
// Nothing of the reference is copied here; the binary is built into a temporary directory and never kept.
//   mesh_attr_ref_driver <cases.txt> <results.txt>
// Every number travels as a C hex float (%a).  One case per line:
//   normals  nv nf v[nv * 14] i[nf * 3]   -> generated v[nv * 14]      (records are the reference's Vertex, model.h:14-20)
//   tangents nv nf v[nv * 14] i[nf * 3]   -> generated v[nv * 14]
// generated: 1 when the function announced its work on std::cout (model.cpp:280,329), which it does exactly when it rewrites.
#define private public          // the two functions and Model::vertices / indices are private (model.h:98-130); access control does not change the layout
#include "model.h"
#undef private

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
const char* Assimp::Importer::GetErrorString() const { return "mesh_attr_ref_driver: no scene"; }

static double num(std::istream& in) { std::string t; in >> t; return std::strtod(t.c_str(), nullptr); }
static void put(std::ostream& out, double d) { char b[64]; std::snprintf(b, sizeof b, "%a ", d); out << b; }

int main(int argc, char** argv) {
    if (argc < 3) return 1;
    static_assert(sizeof(Vertex) == 14 * sizeof(double), "Vertex is 14 packed doubles");
    std::ifstream in(argv[1]);
    std::ofstream out(argv[2]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string what; ls >> what;
        if (what.empty()) continue;
        if (what != "normals" && what != "tangents") { std::fprintf(stderr, "mesh_attr_ref_driver: unknown case '%s'\n", what.c_str()); return 2; }
        size_t nv, nf; ls >> nv >> nf;
        Model model("mesh_attr_ref_driver.obj");
        model.vertices.resize(nv);
        double* rec = reinterpret_cast<double*>(model.vertices.data());
        for (size_t k = 0; k < nv * 14; ++k) rec[k] = num(ls);
        model.indices.resize(nf * 3);
        for (size_t k = 0; k < nf * 3; ++k) { unsigned long i; ls >> i; model.indices[k] = (unsigned int)i; }
        if (!ls) { std::fprintf(stderr, "mesh_attr_ref_driver: short case\n"); return 2; }
        std::ostringstream said;
        std::streambuf* keep = std::cout.rdbuf(said.rdbuf());
        if (what == "normals") model.generateNormalsIfNeeded(); else model.computeTangentsIfNeeded();
        std::cout.rdbuf(keep);
        out << (said.str().empty() ? 0 : 1) << " ";
        rec = reinterpret_cast<double*>(model.vertices.data());
        for (size_t k = 0; k < nv * 14; ++k) put(out, rec[k]);
        out << "\n";
    }
    return out ? 0 : 3;
}
