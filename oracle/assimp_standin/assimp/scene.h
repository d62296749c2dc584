// Stand-in for <assimp/scene.h> — TEST INFRASTRUCTURE, NOT PRODUCT.
//
// Declarations only.  The reference's model.h includes Assimp, which is not available where the oracle is
// built; these headers declare just the names the reference's model.cpp uses, so that its Model::load,
// samplers and the shaders of main.cpp can be compiled and driven by oracle/ref_shaders.cpp.  No Assimp
// behaviour is exercised: Importer::ReadFile (defined in ref_shaders.cpp) hands back a scene the harness
// filled in itself, and no post-processing step (aiProcess_*) is applied.
#pragma once

enum aiTextureType {
    aiTextureType_NONE = 0, aiTextureType_DIFFUSE = 1, aiTextureType_SPECULAR = 2, aiTextureType_AMBIENT = 3,
    aiTextureType_EMISSIVE = 4, aiTextureType_HEIGHT = 5, aiTextureType_NORMALS = 6,
};
enum aiReturn { aiReturn_SUCCESS = 0, aiReturn_FAILURE = -1 };
#define AI_SUCCESS aiReturn_SUCCESS
#define AI_SCENE_FLAGS_INCOMPLETE 0x1

struct aiVector3D { float x = 0, y = 0, z = 0; };

struct aiString {
    char data[1024] = { 0 };
    const char* C_Str() const { return data; }
};

struct aiFace { unsigned int mNumIndices = 0; unsigned int* mIndices = nullptr; };

// No textures: GetTextureCount() is 0 for every type, which sends Model::loadTexture to its <stem><suffix>.tga fallback.
struct aiMaterial {
    unsigned int GetTextureCount(aiTextureType) const { return 0; }
    aiReturn GetTexture(aiTextureType, unsigned int, aiString*) const { return aiReturn_FAILURE; }
};

struct aiMesh {
    aiString mName;
    unsigned int mMaterialIndex = 0;
    unsigned int mNumVertices = 0, mNumFaces = 0;
    aiVector3D* mVertices = nullptr;
    aiVector3D* mNormals = nullptr;
    aiVector3D* mTangents = nullptr;
    aiVector3D* mBitangents = nullptr;
    aiVector3D* mTextureCoords[8] = { nullptr };
    aiFace* mFaces = nullptr;
    bool HasNormals() const { return mNormals != nullptr; }
    bool HasTextureCoords(unsigned int i) const { return i < 8 && mTextureCoords[i] != nullptr; }
    bool HasTangentsAndBitangents() const { return mTangents != nullptr && mBitangents != nullptr; }
};

struct aiNode {
    unsigned int mNumMeshes = 0; unsigned int* mMeshes = nullptr;
    unsigned int mNumChildren = 0; aiNode** mChildren = nullptr;
};

struct aiScene {
    unsigned int mFlags = 0;
    aiNode* mRootNode = nullptr;
    unsigned int mNumMeshes = 0; aiMesh** mMeshes = nullptr;
    unsigned int mNumMaterials = 0; aiMaterial** mMaterials = nullptr;
    bool HasMaterials() const { return mNumMaterials > 0; }
};
