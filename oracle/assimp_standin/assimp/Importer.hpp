// Stand-in for <assimp/Importer.hpp> — TEST INFRASTRUCTURE, NOT PRODUCT.  Declarations only (see scene.h): the
// three members the reference's model.cpp calls.  Their definitions live in oracle/ref_shaders.cpp and return the
// scene that harness built; no file is parsed and no Assimp behaviour is exercised.
#pragma once
#include <string>
#include "scene.h"

namespace Assimp {
class Importer {
public:
    const aiScene* ReadFile(const std::string& file, unsigned int flags);
    void FreeScene();
    const char* GetErrorString() const;
};
}  // namespace Assimp
