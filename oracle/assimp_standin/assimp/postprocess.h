// Stand-in for <assimp/postprocess.h> — TEST INFRASTRUCTURE, NOT PRODUCT.  Declarations only (see scene.h):
// the flag names the reference's model.cpp passes to ReadFile.  No post-processing step is applied.
#pragma once

enum aiPostProcessSteps {
    aiProcess_CalcTangentSpace = 0x1, aiProcess_JoinIdenticalVertices = 0x2, aiProcess_Triangulate = 0x8,
    aiProcess_GenNormals = 0x20, aiProcess_ValidateDataStructure = 0x400, aiProcess_ImproveCacheLocality = 0x800,
    aiProcess_OptimizeMeshes = 0x200000, aiProcess_FlipUVs = 0x800000,
};
