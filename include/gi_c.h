/*
 * gi_c.h -- C ABI of the MI355X-native render core ("libgatling_gi.so").
 *
 * This is the drop-in boundary for the path BASELINE.json names: the `gi` render loop of
 * pablode/gatling.  In the reference that boundary is the C++ API of
 * /root/reference/src/gi/gtl/gi/Gi.h:199-261 (free functions over opaque structs, linked as a static
 * library into hdGatling.so).  Every entry point below cites the Gi.h declaration it replaces; argument
 * meaning, ownership and error behaviour follow the reference:
 *   - the library owns every handle; callers destroy explicitly;
 *   - giCCreateMesh COPIES all vertex/face data before returning (Gi.cpp:620-638);
 *   - transforms are row-major 4x4 floats in USD's row-vector convention (Gi.cpp:641-658);
 *   - setters only mark the scene dirty; BVH build + upload happen in the next giCRender
 *     (hdGatling/renderDelegate.cpp:208-213);
 *   - giCRender blocks until the AOVs are complete in host memory (Gi.cpp:2492-2502);
 *   - status returns: GI_C_OK / GI_C_ERROR; creators return NULL on failure; no exceptions cross.
 * Differences, all forced by plain-C types: std::vector / std::string_view arguments become
 * pointer + count; MaterialX/MDL material creation (Gi.h:204-206) becomes giCCreateMaterial with a
 * closed-form parameter block (DESIGN.md "Materials"); the gtl:: C++ shim on top of this header lives in
 * include/gtl/gi/Gi.h.  Extensions that the reference does not have are marked [ext].
 *
 * The library is HIP-only: if no gfx950 device / HIP runtime is available giCInitialize fails
 * (there is no CPU fallback).
 */
#ifndef GATLING_GI_C_H
#define GATLING_GI_C_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GI_C_OK 0
#define GI_C_ERROR 1

#define GI_C_MAX_AOV_COMP_SIZE 16 /* Gi.h:32 */

/* Gi.h:36-56 */
typedef enum GiCAovId {
  GI_C_AOV_COLOR = 0, GI_C_AOV_NORMAL, GI_C_AOV_NEE, GI_C_AOV_BARYCENTRICS, GI_C_AOV_TEXCOORDS, GI_C_AOV_BOUNCES,
  GI_C_AOV_CLOCK_CYCLES, GI_C_AOV_OPACITY, GI_C_AOV_TANGENTS, GI_C_AOV_BITANGENTS, GI_C_AOV_THIN_WALLED,
  GI_C_AOV_OBJECT_ID, GI_C_AOV_DEPTH, GI_C_AOV_FACE_ID, GI_C_AOV_INSTANCE_ID, GI_C_AOV_DOUBLE_SIDED, GI_C_AOV_ALBEDO,
  GI_C_AOV_COUNT
} GiCAovId;

/* [ext] Sample moments: an id a GiCAovBinding takes beside the GiCAovId values.  It lies OUTSIDE the enum: GI_C_AOV_COUNT stays 17 and the enum keeps mirroring
 * Gi.h.  The buffer is Float32Vec4 and holds, per pixel, M = (S1, S2, n, 0) over the samples the colour AOV's running accumulation holds:
 *   L = (0.2126 r + 0.7152 g) + 0.0722 b of a path sample as the colour pass retires it (after the clamp to maxSampleValue), no fused multiply-add;
 *   S1 = sum of L, S2 = sum of (L L), n = sum of 1.0f, the samples added one by one in sample order, from zero (gi_moments.h).
 * M depends on the samples alone: N progressive calls of spp 1, one call of spp N, a call cut into batches (GI_C_SCENE_OPTION_SAMPLE_BUFFER_MB), look-ahead
 * windows (the moments ride along: the binding does not switch look-ahead off) and a row share give the same bytes for the rows they render; rows outside a
 * call's share are not written.  The binding's clear value is not used.  Whatever resets the colour's accumulation (a camera or settings change, an edit,
 * progressiveAccumulation off) restarts M at that call.  A buffer first bound at a sample offset > 0 -- or bound again after a call that did not bind it --
 * starts from zero at that call: its n then counts fewer samples than the colour holds.  A binding without a colour binding renders the colour pass into
 * scratch memory, as the path-following AOVs do.  Multi-device renders: every device accumulates its rows in its own copy and the shares are gathered into
 * the primary's buffer exactly as the colour AOV's are.  Without the binding giCRender launches what it launched before: the kernel (gi_moments.hip
 * k_moments, one thread per pixel, beside each batch's accumulation) runs for renders that bind it alone. */
#define GI_C_AOV_EXT_MOMENTS 0x100

/* Gi.h:70-75 */
typedef enum GiCRenderBufferFormat { GI_C_FORMAT_INT32 = 0, GI_C_FORMAT_FLOAT32 = 1, GI_C_FORMAT_FLOAT32_VEC4 = 2 } GiCRenderBufferFormat;

typedef struct GiCScene GiCScene;
typedef struct GiCMaterial GiCMaterial;
typedef struct GiCMesh GiCMesh;
typedef struct GiCSphereLight GiCSphereLight;
typedef struct GiCDistantLight GiCDistantLight;
typedef struct GiCRectLight GiCRectLight;
typedef struct GiCDiskLight GiCDiskLight;
typedef struct GiCDomeLight GiCDomeLight;
typedef struct GiCRenderBuffer GiCRenderBuffer;

/* Gi.h:96-108 (same layout) */
typedef struct GiCCameraDesc {
  float position[3];
  float forward[3];
  float up[3];
  float vfov;
  float fStop;
  float focusDistance;
  float focalLength;
  float clipStart;
  float clipEnd;
  float exposure;
} GiCCameraDesc;

/* Gi.h:110-118 (same layout, 48 bytes) */
typedef struct GiCVertex {
  float pos[3];
  float u;
  float norm[3];
  float v;
  float tangent[3];
  float bitangentSign;
} GiCVertex;

/* Gi.h:120-122 */
typedef struct GiCFace { uint32_t v_i[3]; } GiCFace;

/* Gi.h:124-137 with vectors flattened to pointer+count; GiMeshDesc.primvars arrive through giCSetMeshPrimvars */
typedef struct GiCMeshDesc {
  uint32_t faceCount;
  const GiCFace* faces;
  const int32_t* faceIds; /* faceCount entries or NULL */
  int32_t id;
  int32_t isDoubleSided;
  int32_t isLeftHanded;
  const char* name;
  uint32_t maxFaceId;
  uint32_t vertexCount;
  const GiCVertex* vertices;
} GiCMeshDesc;

/* Gi.h:139-159 (bools widened to int32 for a stable ABI) */
typedef struct GiCRenderSettings {
  int32_t clippingPlanes;
  int32_t depthOfField;
  int32_t domeLightCameraVisible;
  int32_t filterImportanceSampling;
  float frame;
  int32_t jitteredSampling;
  float lightIntensityMultiplier;
  uint32_t maxBounces;
  float maxSampleValue;
  uint32_t maxVolumeWalkLength;
  uint32_t mediumStackSize;
  float metersPerSceneUnit;
  int32_t nextEventEstimation;
  int32_t progressiveAccumulation;
  uint32_t rrBounceOffset;
  float rrInvMinTermProb;
  uint32_t spp;
  float time;
} GiCRenderSettings;

/* Gi.h:161-166 */
typedef struct GiCAovBinding {
  int32_t aovId; /* GiCAovId */
  uint8_t clearValue[GI_C_MAX_AOV_COMP_SIZE];
  GiCRenderBuffer* renderBuffer;
} GiCAovBinding;

/* Gi.h:168-175 */
typedef struct GiCRenderParams {
  const GiCAovBinding* aovBindings;
  uint32_t aovBindingCount;
  GiCCameraDesc camera;
  GiCDomeLight* domeLight;
  GiCRenderSettings renderSettings;
  GiCScene* scene;
  /* Non-colour AOVs: Normal, Barycentrics, Texcoords, Opacity, Tangents, Bitangents, ThinWalled, ObjectId, Depth, FaceId, InstanceId,
   * DoubleSided and Albedo are produced by a primary-hit pass (vec3 AOVs need Float32Vec4 buffers, Depth Float32, ids Int32 --
   * Gi.cpp:302-316); NEE, Bounces and ClockCycles follow whole paths and are filled by the colour pass (which then runs even without a
   * Color binding).  ClockCycles is a Turbo heat map, normalised to the frame maximum, alpha 255 (_EncodeRenderBufferAsHeatmap,
   * Gi.cpp:327-343) of a deterministic cost proxy -- the ray segments traced for the pixel -- instead of the shader clock. */
  /* [ext] multi-GPU sharding: render only image rows [rowBegin,rowEnd) of the full image whose size is the
   * render buffers' size; rowEnd == 0 means "all rows".  RNG streams use the global pixel index so an N-way
   * split is bit-identical to the single-GPU image. */
  uint32_t rowBegin;
  uint32_t rowEnd;
  /* [ext] rows rowBegin, rowBegin + rowStride, ... below rowEnd (0 and 1 mean every row).  Rank r of N rendering
   * (rowBegin = r, rowEnd = height, rowStride = N) gets an even share of cheap and expensive image regions: on the cornell frame
   * contiguous eighths differ by 0.61x .. 1.19x of the mean cost. */
  uint32_t rowStride;
} GiCRenderParams;

/* Closed-form material classes: replaces MaterialX->MDL->GLSL codegen (src/mc, GlslShaderGen) */
#define GI_C_MAT_DIFFUSE 0u             /* config C1 "diffuse only" model */
#define GI_C_MAT_USD_PREVIEW_SURFACE 1u /* diffuse + GGX specular + clearcoat */
#define GI_C_MAT_OPEN_PBR 2u             /* coat + metal (F82-tint) + dielectric reflection + rough refraction + diffuse */
#define GI_C_MAT_PARAM_COUNT 64u
/* indices into GiCMaterialDesc.p */
#define GI_C_P_BASE_COLOR 0
#define GI_C_P_EMISSION 3
#define GI_C_P_USE_SPECULAR_WORKFLOW 6
#define GI_C_P_SPECULAR_COLOR 7
#define GI_C_P_METALLIC 10
#define GI_C_P_ROUGHNESS 11
#define GI_C_P_CLEARCOAT 12
#define GI_C_P_CLEARCOAT_ROUGHNESS 13
#define GI_C_P_OPACITY 14
#define GI_C_P_OPACITY_THRESHOLD 15
#define GI_C_P_IOR 16
#define GI_C_P_BASE_WEIGHT 17
#define GI_C_P_SPECULAR_WEIGHT 18
#define GI_C_P_COAT_COLOR 19
#define GI_C_P_COAT_IOR 22
#define GI_C_P_TRANSMISSION_WEIGHT 23
#define GI_C_P_TRANSMISSION_COLOR 24
#define GI_C_P_DIFFUSE_ROUGHNESS 27
#define GI_C_P_TRANSMISSION_DEPTH 28
#define GI_C_P_TRANSMISSION_SCATTER 29 /* 3: OpenPBR transmission_scatter (open_pbr_surface.mtlx:35) */
#define GI_C_P_TRANSMISSION_SCATTER_ANISOTROPY 47 /* transmission_scatter_anisotropy (:37); slots 38..46 are reserved (32..37: subsurface radius, coat / specular rotation) */
#define GI_C_P_COAT_DARKENING 48   /* OpenPBR coat_darkening (open_pbr_surface.mtlx:64; default 1): strength of the base darkening under the coat (:470-541) */
#define GI_C_P_FUZZ_WEIGHT 49      /* OpenPBR fuzz_weight / fuzz_color (3) / fuzz_roughness (:57-59): the fuzz (sheen) layer over the coat (:569-581) */
#define GI_C_P_FUZZ_COLOR 50
#define GI_C_P_FUZZ_ROUGHNESS 53
#define GI_C_P_SUBSURFACE_WEIGHT 55  /* OpenPBR subsurface_weight (open_pbr_surface.mtlx:43, 213-218); modelled for thin-walled materials (:140-196), else treated as 0 */
#define GI_C_P_SUBSURFACE_COLOR 56   /* 3: subsurface_color (:45), default 0.8 */
#define GI_C_P_SUBSURFACE_ANISOTROPY 59 /* subsurface_scatter_anisotropy (:51) */
#define GI_C_P_THIN_FILM_WEIGHT 62    /* OpenPBR thin_film_weight (open_pbr_surface.mtlx:71, 426-431, 461-464): mixes a thin film's interference into the Fresnel factor of the dielectric and metal lobes */
#define GI_C_P_THIN_FILM_THICKNESS 63 /* thin_film_thickness in micrometres (:73, 300-304), default 0.5 */
#define GI_C_P_THIN_FILM_IOR 6        /* thin_film_ior (:75), default 1.4 -- OpenPBR class only: the slot is useSpecularWorkflow for UsdPreviewSurface */
#define GI_C_P_SPECULAR_ANISOTROPY 60 /* OpenPBR specular_roughness_anisotropy (open_pbr_surface.mtlx:27, 133-136): GGX stretched along the tangent, alpha_t = r^2 sqrt(2 / (1 + (1 - a)^2)), alpha_b = (1 - a) alpha_t */
#define GI_C_P_COAT_ANISOTROPY 61     /* coat_roughness_anisotropy (:65, 552-555), along the coat's tangent: see GI_C_P_COAT_ROTATION */
#define GI_C_P_COAT_ROTATION 36       /* OpenPBR geometry_coat_tangent (open_pbr_surface.mtlx:91, 561) in the form documents bind it: the geometry tangent turned by this many
                                         TURNS (1 = 360 degrees) towards the bitangent, about the coat's normal (rotate3d of Tworld; Standard Surface's coat_rotation).
                                         0 = the geometry tangent.  Read for an anisotropic coat only (coat weight and coat_roughness_anisotropy > 0).  Like 32..35 an input
                                         of the USER block only (API version 7) */
#define GI_C_P_SPECULAR_ROTATION 37   /* OpenPBR geometry_tangent (open_pbr_surface.mtlx:89; the tangent of the dielectric and conductor lobes, :385 ... 457) in the same form:
                                         the geometry tangent turned by this many turns towards the bitangent (Standard Surface's specular_rotation; glTF's anisotropy_rotation
                                         / 2 pi).  Read for anisotropic base lobes only (specular_roughness_anisotropy > 0); the coat keeps the geometry tangent and its own
                                         turn.  USER block only (API version 7; slots 38..46 stay reserved) */
#define GI_C_P_SUBSURFACE_RADIUS 32       /* OpenPBR subsurface_radius (open_pbr_surface.mtlx:47, default 1): with _RADIUS_SCALE the per-channel mean free path of the volumetric
                                            subsurface_bsdf (:182-192) of materials that are not thin-walled; live in renders with a medium stack (mediumStackSize > 0) */
#define GI_C_P_SUBSURFACE_RADIUS_SCALE 33 /* 3 floats, subsurface_radius_scale (:49, default 1, 0.5, 0.25).  Slots 32..35 are inputs of the USER block only: the device copy of a
                                            material keeps derived constants at these indices (written after the inputs were read).  Taken as given: zeros are zeros (the mean free path is clamped to
                                            1e-6 per channel); the OpenPBR defaults are the front ends' to set (gtl_shim.cpp does; API version 6) */
#define GI_C_P_THIN_WALLED 54      /* OpenPBR geometry_thin_walled (:88) != 0: MDL thin_walled semantics (rp_main.chit:153-157, 188-189, 447) */

/* Note: p[GI_C_P_OPACITY] is the cutout opacity (1 = opaque); a zero-filled block is a fully transparent material. */
typedef struct GiCMaterialDesc {
  uint32_t klass;
  uint32_t flags;
  float p[GI_C_MAT_PARAM_COUNT];
} GiCMaterialDesc;

/* [ext] Textures.  The reference loads images by file path inside gi (TextureManager.cpp:100-275 through imgio's PNG / JPEG /
 * EXR / HDR / TIFF decoders, which are out of scope here) and samples them through the MDL renderer runtime
 * (mdl_interface.glsl:8-38, 127-145).  This boundary takes DECODED pixels: linear float RGBA, row 0 first (the v = 0 side);
 * the pixels are copied.  Lookups are bilinear, LOD 0, after the runtime's wrap handling. */
typedef struct GiCTexture GiCTexture;
typedef struct GiCTextureDesc { uint32_t width, height; const float* rgba; } GiCTextureDesc;
GiCTexture* giCCreateTexture(GiCScene* scene, const GiCTextureDesc* desc);
/* [ext] decodes .png (8/16-bit, non-interlaced), baseline / extended-sequential .jpg (Huffman, 8-bit, grey or YCbCr, any subsampling,
 * restart intervals; progressive files are refused), .hdr or .pfm in-library; srgbToLinear applies the sRGB EOTF to 8-bit colour;
 * a (path, srgbToLinear) pair that is already loaded and alive returns the SAME handle with one more reference (the file cache of
 * TextureManager.cpp:100-150); giCDestroyTexture releases one reference */
GiCTexture* giCCreateTextureFromFile(GiCScene* scene, const char* filePath, int32_t srgbToLinear);
/* [ext] the decoder alone (no device needed; tests): returns 1 and fills width/height (+ rgba if it holds width*height*4 floats).  Goes through the registered
 * asset reader and image loader like giCCreateTextureFromFile / giCCreateDomeLight do. */
int giCDebugDecodeImage(const char* filePath, int32_t srgbToLinear, uint32_t* width, uint32_t* height, float* rgba, uint64_t rgbaFloats);

/* Asset reader -- replaces gtl::GiAssetReader (/root/reference/src/gi/gtl/gi/Gi.h:186-194, giRegisterAssetReader :201).  The reference reads EVERY image through it
 * (TextureManager.cpp:39-52 `_ReadImage`: open -> size -> data -> decode -> close; hdGatling registers an ArResolver-backed one, rendererPlugin.cpp:95-143, 189), so
 * paths a plain fopen cannot serve -- usdz package members, URI resolvers, search-path relative names -- load.  With a reader registered the library opens image
 * `filePath`s (giCCreateTextureFromFile, giCCreateDomeLight, giCDebugDecodeImage) through it and never touches the file system for them; with none (the default, or
 * after giCRegisterAssetReader(NULL)) it reads the file itself.  The struct is copied.  `open` returns an opaque asset or NULL; `data` stays valid until `close`. */
typedef struct GiCAssetReader {
  void* user;
  void* (*open)(void* user, const char* path);
  uint64_t (*size)(void* user, void* asset);
  const void* (*data)(void* user, void* asset);
  void (*close)(void* user, void* asset);
} GiCAssetReader;
void giCRegisterAssetReader(const GiCAssetReader* reader);

/* Image loader hook -- the reference decodes image bytes with imgio (`ImgioLoadImage(data, size, &img, flags)`, TextureManager.cpp:48; PNG, JPEG incl. progressive,
 * EXR, HDR, TIFF), which is outside this library (imgio stays as-is on the reference side).  The library's own decoders cover .png, baseline .jpg,
 * .hdr and .pfm; a registered loader is asked FIRST for every image (bytes from the asset reader or the file), so a host that has imgio hands EXR / TIFF / progressive
 * JPEG over through it.  `load` returns 1 and fills `out` (pixels in imgio's orientation: row 0 = the picture's BOTTOM scanline) or 0 = "not mine", in which case the
 * in-library decoders are tried; `release` is called once for every successful `load` after the pixels have been copied.  keepHdr mirrors ImgioLoadFlags::KeepHdr
 * (set for dome lights, Gi.cpp:2215-2230).  8-bit data is unorm; the sRGB EOTF is applied by the library when the texture was created with srgbToLinear. */
#define GI_C_IMAGE_RGBA8_UNORM 1   /* imgio ImgioFormat::RGBA8_UNORM  */
#define GI_C_IMAGE_RGB16_FLOAT 2   /*       ImgioFormat::RGB16_FLOAT  */
#define GI_C_IMAGE_RGBA16_FLOAT 3  /*       ImgioFormat::RGBA16_FLOAT */
#define GI_C_IMAGE_R32_FLOAT 4     /*       ImgioFormat::R32_FLOAT    */
#define GI_C_IMAGE_RGBA32_FLOAT 5  /* [ext] */
typedef struct GiCDecodedImage { uint32_t format, width, height, reserved; const void* pixels; void* handle; } GiCDecodedImage;
typedef struct GiCImageLoader {
  void* user;
  int32_t (*load)(void* user, const char* path, const void* bytes, uint64_t size, int32_t keepHdr, GiCDecodedImage* out);
  void (*release)(void* user, GiCDecodedImage* image);
} GiCImageLoader;
void giCSetImageLoader(const GiCImageLoader* loader); /* NULL: in-library decoders only (the default) */
void giCDestroyTexture(GiCTexture* texture);

/* texturable inputs of the closed-form materials (UsdUVTexture semantics: value = texel * scale + bias at the hit's st) */
#define GI_C_TEX_BASE_COLOR 0 /* diffuseColor / base_color (rgb) */
#define GI_C_TEX_EMISSION 1   /* emissiveColor / emission (rgb)  */
#define GI_C_TEX_ROUGHNESS 2  /* scalar: `channel` of the texel  */
#define GI_C_TEX_METALLIC 3   /* scalar                          */
#define GI_C_TEX_NORMAL 4     /* tangent-space normal (rgb, usually scale 2 bias -1); bent by mdl_adapt_normal (mdl_interface.glsl:238-256) */
#define GI_C_TEX_OPACITY 5    /* scalar: cutout opacity (UsdPreviewSurface opacity / OpenPBR geometry_opacity), evaluated per candidate hit by the any-hit test (rp_main.ahit:51-60); texture only */
#define GI_C_TEX_COAT_NORMAL 6 /* vector: OpenPBR geometry_coat_normal (open_pbr_surface.mtlx:87, 560), a tangent-space normal map for the coat lobe's own shading frame (OpenPBR class only) */
#define GI_C_TEX_TRANSMISSION_WEIGHT 7 /* scalar: OpenPBR transmission_weight (open_pbr_surface.mtlx:29) */
#define GI_C_TEX_TRANSMISSION_COLOR 8  /* rgb: OpenPBR transmission_color (:31) -- the surface tint when transmission_depth is 0; with a depth the colour defines the MEDIUM's absorption,
                                         * which stays the material's constant (a path's medium is pushed once, where it enters) */
#define GI_C_TEX_SLOT_COUNT 9
#define GI_C_TEX_WRAP_CLAMP 0 /* mdl_types.glsl:117-120 */
#define GI_C_TEX_WRAP_REPEAT 1
#define GI_C_TEX_WRAP_MIRRORED_REPEAT 2
#define GI_C_TEX_WRAP_CLIP 3
typedef struct GiCTextureBinding {
  GiCTexture* texture; /* NULL removes the binding */
  int32_t wrapS, wrapT;
  int32_t channel;
  float scale[4], bias[4];
} GiCTextureBinding;
int giCSetMaterialTexture(GiCMaterial* material, int32_t input, const GiCTextureBinding* binding);
/* [ext] Texture-coordinate transform of an input's lookup: s' = (xf[0] s + xf[1] t) + xf[2], t' = (xf[3] s + xf[4] t) + xf[5]; NULL = identity.  What a UsdTransform2d
 * node between the primvar reader and a UsdUVTexture's `st` means (UsdPreviewSurface specification: result = in * scale, rotated counter-clockwise by `rotation`
 * degrees, + translation: xf = {c sx, -s sy, tx, s sx, c sy, ty}); the reference compiles the node through MaterialX -> MDL (src/mc/impl/MtlxMdlCodeGen.cpp:186-215),
 * the gtl shim's MaterialX reader folds it into these six floats. */
int giCSetMaterialTextureTransform(GiCMaterial* material, int32_t input, const float* xf);

/* Scene data (primvars).  Gi.h:76-92: GiPrimvarData with the byte vector flattened to pointer + size; data = 4-byte elements (float, or int32 for
 * the Int types).  A material input bound to a primvar NAME reads the primvar of the hit mesh (instancer primvars first, mesh primvars
 * override, Gi.cpp:913-929) through scene_data_lookup_float3 / _float (mdl_interface.glsl:281-301, 337-424): barycentric blend of the
 * three vertex values, or the uniform / instance / constant value; integer primvars go through scene_data_lookup_int (:426-476): the
 * value of the NEAREST vertex (largest barycentric weight), converted to float.  The names "CAMERA_POSITION" (colour inputs) and
 * "FRAME" (scalar inputs) are answered from the camera / GiCRenderSettings.frame like the reference's UBO short cuts (:329-334,
 * 390-395).  A mesh without that primvar keeps the input's constant.  A texture on the same input takes precedence. */
#define GI_C_PRIMVAR_FLOAT 0
#define GI_C_PRIMVAR_VEC2 1
#define GI_C_PRIMVAR_VEC3 2
#define GI_C_PRIMVAR_VEC4 3
#define GI_C_PRIMVAR_INT 4
#define GI_C_PRIMVAR_INT2 5
#define GI_C_PRIMVAR_INT3 6
#define GI_C_PRIMVAR_INT4 7
#define GI_C_INTERP_CONSTANT 0
#define GI_C_INTERP_INSTANCE 1
#define GI_C_INTERP_UNIFORM 2
#define GI_C_INTERP_VERTEX 3
typedef struct GiCPrimvarData { const char* name; int32_t type; int32_t interpolation; const void* data; uint64_t dataSize; } GiCPrimvarData;
int giCSetMeshPrimvars(GiCMesh* mesh, uint32_t count, const GiCPrimvarData* primvars);          /* GiMeshDesc.primvars (Gi.h:134) */
int giCSetMeshInstancerPrimvars(GiCMesh* mesh, uint32_t count, const GiCPrimvarData* primvars); /* Gi.h:213 */
int giCSetMaterialPrimvarInput(GiCMaterial* material, int32_t input, const char* primvarName);  /* [ext] NULL or "" removes it; inputs: base colour, emission, roughness, metalness, transmission weight / colour (not the normal, opacity and coat-normal slots: texture only) */

/* [ext] per-frame statistics of the last giCRender on a scene (measurement) */
typedef struct GiCRenderStats {
  double renderMs;       /* wall time of the bounce loop incl. final D2H of the colour AOV */
  double bvhBuildMs;     /* BVH8 build on whichever side ran it, host or device (GI_C_SCENE_OPTION_BVH_BUILD); 0 if not rebuilt */
  double uploadMs;       /* scene upload (0 if not rebuilt)                                 */
  double traceMs;        /* sum of closest-hit traversal kernel time (HIP events)           */
  double shadeMs;        /* sum of shade kernel time                                        */
  double raygenMs;       /* sum of raygen/accumulate kernel time                            */
  double shadowMs;       /* sum of shadow traversal kernel time                             */
  uint64_t samples;      /* pixels * spp rendered by this call                              */
  uint64_t segments;     /* closest-hit rays traced                                         */
  uint64_t shadowRays;   /* shadow rays traced                                              */
  uint64_t nodesVisited; /* BVH8 nodes fetched by closest-hit traversal (if counting on)    */
  uint64_t trisTested;   /* triangles tested by closest-hit traversal (if counting on)      */
  uint64_t shadowNodesVisited;
  uint64_t shadowTrisTested;
  uint32_t iterations;   /* wavefront iterations                                            */
  uint32_t traceLaunches;
  uint32_t nodeCount;    /* BVH8 nodes                                                      */
  uint32_t triangleCount;
  uint32_t fusedPath;    /* 1: the colour pass ran as the fused persistent kernel k_path (LDS-resident scene) */
  uint32_t batches;      /* sample batches the frame was cut into (per-sample colour buffer budget; memory plan of giCRender) */
  uint32_t poolSlots;    /* slots of the persistent path pool this render used (0: fused kernel)                              */
  uint32_t inactiveTriangleCount; /* instanced triangles left out of the BVH: a non-finite or out-of-range (> 1e18) vertex, a non-invertible transform (was reserved0) */
} GiCRenderStats;
/* With GI_C_SCENE_OPTION_SAMPLE_LOOKAHEAD the counts and stage times (segments, shadowRays, the node / triangle counters, iterations, traceLaunches, batches,
 * poolSlots, fusedPath, traceMs ...) describe the work the call LAUNCHED: the whole window for a call that traced one, zero for a call that was served from it.
 * `samples` stays the call's own pixels * spp and `renderMs` its own wall time.  Summed over the calls of a window, segments / shadowRays are what the same calls
 * count without look-ahead. */

/* [ext] sample look-ahead (GI_C_SCENE_OPTION_SAMPLE_LOOKAHEAD) as the last giCRender on the scene left it (of a multi-device render: the primary device's share;
 * every device looks ahead for its own rows, in step) */
typedef struct GiCLookaheadStats {
  uint32_t windowCalls;      /* calls the current window holds (1: the call traced itself alone; 0: no window -- look-ahead off or declined by this call) */
  uint32_t windowServed;     /* calls of it served so far, this one included                                                                              */
  uint32_t traced;           /* 1: this call traced (its window, or itself as without look-ahead); 0: it was served without tracing a ray                 */
  uint32_t reserved;
  uint64_t windowsTraced;    /* since the scene was created: windows traced (those of one call included) ...                                              */
  uint64_t callsServed;      /* ... calls served without tracing ...                                                                                      */
  uint64_t windowsDiscarded; /* ... windows dropped while they still held calls nobody had asked for (an edit, another size, released memory) ...         */
  uint64_t samplesUnused;    /* ... and the samples per pixel traced for those calls                                                                      */
} GiCLookaheadStats;

/* Gi.h:199-200.  deviceOrdinal selects the HIP device (the reference picks one Vulkan device by score,
 * CgpuVk.cpp:892-909).  One giCInitialize per process, like the reference's global state (Gi.cpp:244-259). */
int giCInitialize(int deviceOrdinal);
void giCTerminate(void);
/* [ext] Multi-device form (north_star: "pixels/samples shard across the 8 GPUs of one node, scene replicated, tiles gathered"; the reference picks ONE
 * device, CgpuVk.cpp:892-909).  The first ordinal is the primary device: render buffers, textures and the single-device entry points live there.  Every
 * giCRender of a whole frame then deals the image rows round-robin to the devices (row r to device r mod N, scene replicated at build time, one host
 * thread per device), and the shares are copied into the primary device's render buffer over xGMI (strided peer copies straight into place) before the
 * one D2H -- the image is bit-identical to a one-device render.  giCInitialize does the same when $GATLING_DEVICES ("0,1,2,3" or "all") is set, which is
 * how an unmodified caller (hdGatling) gets every GPU of the node.  Renders that shard rows themselves (rowStride > 1 / a row range) stay on the primary. */
int giCInitializeDevices(const int32_t* deviceOrdinals, uint32_t count);
/* [ext] Version of this header's ABI: bumped whenever a struct grows or an entry point changes meaning (5: GiCRenderStats gained batches / poolSlots, GI_C_TEX_SLOT_COUNT 9,
 * the subsurface radius slots of GiCMaterialDesc, the asset-reader / image-loader hooks; 6: GiCRenderStats.reserved0 became inactiveTriangleCount,
 * giCDebugShadeClass, an all-zero subsurface radius is no longer read as "unset", the hostile-input rules above giCRender;
 * 7: GI_C_P_COAT_ROTATION / GI_C_P_SPECULAR_ROTATION, slots that were reserved; 8: GI_C_SCENE_OPTION_BVH_BUILD, giCDebugValidateSceneBvh, bvhBuildMs counts
 * the device build when one ran).  A caller compares giCGetApiVersion() with the GI_C_API_VERSION it was built with.
 * Still 8 with GI_C_SCENE_OPTION_SAMPLE_LOOKAHEAD and giCGetLookaheadStats: no struct grew and no entry point changed meaning -- both are additions that a caller
 * built against an earlier header never sees.  A caller probes for them: giCSetSceneOption answers GI_C_ERROR for an option the library does not know.
 * The same holds for GI_C_SCENE_OPTION_VISIBILITY_UPDATES, giCDebugSceneVisibilityUpdateCount, giCDebugSceneClassState, giCDebugMissRect and giCDebugPathWalkStats, and for
 * giCSetMeshVertices, GI_C_SCENE_OPTION_VERTEX_UPDATES, giCDebugSceneVertexUpdateCount, giCDebugRefitBvh and giCDebugSceneRefitCheck, and for
 * GI_C_SCENE_OPTION_TOPOLOGY_UPDATES and giCDebugSceneTopologyUpdateCount, and for GI_C_SCENE_OPTION_RESYNC_REFITS, giCDebugSceneResyncCount,
 * giCDebugGatherShade and giCDebugSceneShadeCheck, and for giCDebugPathLobeStats, giCDebugPathRingStats and giCDebugPathLot, and for GI_C_SCENE_OPTION_INSTANCE_UPDATES,
 * giCDebugSceneInstanceUpdateCount and giCDebugCloneInstance, and for GI_C_SCENE_OPTION_TLAS_UPDATES, giCDebugSceneTlasUpdateCount, giCDebugSceneTlasCheck
 * and giCDebugInstanceBounds, and for GI_C_SCENE_OPTION_BLAS_UPDATES, giCDebugSceneBlasUpdateCount, giCDebugSceneBlasCheck, giCDebugBlasRefit and
 * giCDebugBlasRefitHost, and for GI_C_SCENE_OPTION_TLAS_VISIBILITY, giCDebugSceneTlasVisibilityUpdateCount, giCDebugSceneFlatIdCheck and
 * giCDebugPatchVisibilityTwoLevel, and for GI_C_SCENE_OPTION_TLAS_ONLY and giCDebugSceneFlatTreeState, and for GI_C_SCENE_OPTION_TLAS_TOPOLOGY,
 * giCDebugSceneTlasTopologyUpdateCount, giCDebugAppendRecords and giCDebugAppendRecordsHost, and for GI_C_SCENE_OPTION_TLAS_INSTANCES,
 * giCDebugSceneTlasInstanceUpdateStats, giCDebugInstanceRecords and giCDebugInstanceRecordsHost, and for giCDebugTraversalStackHigh and giCDebugBvhStackReach,
 * and for GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD, giCDebugBuildTlasHost, giCDebugBuildTlas and giCDebugSceneTlasBuildStats, and for giCDebugSceneUpsPlain and
 * giCDebugUpsTraits, and for GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD, giCDebugBuildBlasHost, giCDebugBuildBlas and giCDebugSceneBlasBuildStats, and for
 * GI_C_SCENE_OPTION_TLAS_COMPACTION, giCDebugSceneCompactionCount, giCDebugCompactRanges and giCDebugCompactRangesHost, and for giCCreateHostRenderBuffer,
 * giCDenoiseDefaults, giCDenoise and giCGetDenoiseStats, and for GI_C_SCENE_OPTION_LEAF_LIFT, giCDebugSceneLeafLift and giCDebugLeafLift, and for
 * GI_C_AOV_EXT_MOMENTS, giCDebugSampleMoments, giCDebugSampleMomentsHost, giCDenoiseVarianceDefaults and giCDenoiseVariance, and for giCDebugSceneNodeCook,
 * giCDebugNodeCook and giCDebugCheckNodeCook. */
#define GI_C_API_VERSION 8u
uint32_t giCGetApiVersion(void);
uint32_t giCGetDeviceCount(void);
/* [ext] can the primary device and device `index` of the list address each other's memory?  1 = yes (peer access enabled both ways, or the same physical device):
 * row shares are gathered with strided peer copies over xGMI; 0 = no, -1 = the query / the enabling failed: that device's shares are staged through pinned host
 * memory by the library (correct, slower).  tools/run_scale.sh prints it next to every multi-device measurement. */
int32_t giCGetDevicePeerAccess(uint32_t index);
/* [ext] last error message of the calling thread's most recent failing call ("" if none) */
const char* giCGetLastError(void);

/* Gi.h:204-207 */
GiCMaterial* giCCreateMaterial(GiCScene* scene, const char* name, const GiCMaterialDesc* desc);
void giCDestroyMaterial(GiCMaterial* mat);

/* Gi.h:209-216 */
GiCMesh* giCCreateMesh(GiCScene* scene, const GiCMeshDesc* desc);
void giCSetMeshTransform(GiCMesh* mesh, const float* mat4x4);
void giCSetMeshInstanceTransforms(GiCMesh* mesh, uint32_t count, const float* transforms /* count x 16 */);
void giCSetMeshInstanceIds(GiCMesh* mesh, uint32_t count, const int32_t* ids);
/* [ext] Material-side edits of a scene that has been rendered do not rebuild it: giCCreateMaterial / giCDestroyMaterial, giCSetMeshMaterial on a mesh that is part
 * of the scene, giCSetMaterialPrimvarInput, giCSetMaterialTexture / TextureTransform, giCCreateTexture / giCDestroyTexture and giCSetMesh(Instancer)Primvars
 * change the material, texture and scene-data tables and one word per flattened triangle, which the next giCRender patches in device memory (flat and two-level
 * layouts, host- or device-built, partitioned or not; GiCRenderStats.bvhBuildMs = 0, uploadMs = the update).  Measured on the
 * 10.24 M-triangle interior (config C5): full build 2 235 + 919 ms, a colour-only replacement of one material 19.7 ms, re-assigning a 40 960-triangle mesh 17.1 ms.
 * The next render rebuilds instead when the scene has fewer than 4096 triangles, when an edit changes WHICH meshes are in the scene (a mesh loses its material --
 * NULL or destroyed -- or one that was left out gets a valid one), with GATLING_OPTIONS=incremental=0, and for every geometry-side edit (mesh creation /
 * destruction, visibility, instance counts and ids). */
void giCSetMeshMaterial(GiCMesh* mesh, GiCMaterial* mat);
void giCSetMeshVisibility(GiCMesh* mesh, int32_t visible);
/* [ext] Replaces the mesh's vertex array (positions, normals, texture coordinates, tangents): the points of a mesh moved, its topology stayed -- a skinned
 * character, a cloth cache, a sculpt stroke.  Faces, face ids, primvars, material and transforms stay.  `vertexCount` must equal the mesh's vertex count:
 * otherwise GI_C_ERROR with a message, and the mesh is unchanged.  The reference has no such entry point (a points-only sync recreates the mesh there and
 * pays one BLAS build).  The edit raises the flags of a geometry edit; what the next giCRender does with it is GI_C_SCENE_OPTION_VERTEX_UPDATES' business. */
int giCSetMeshVertices(GiCMesh* mesh, uint32_t vertexCount, const GiCVertex* vertices);
void giCDestroyMesh(GiCMesh* mesh);

/* Gi.h:218 */
/* Hostile input (round 6; tests/test_hostile_inputs.py).  The reference copies what Hydra hands it (giCreateMesh, Gi.cpp:628) and leaves the rest to the Vulkan driver,
 * which ignores inactive primitives (CgpuVk.cpp:2561-2670); this library builds its own BVH, so it states its rules:
 *   - a triangle with a vertex that is not finite or lies beyond 1e18 in magnitude AFTER the instance transform is inactive: left out of the BVH, never hit, its
 *     scene-order id kept (FaceId / ObjectId / InstanceId AOVs and giCTraceRays answers do not shift); one warning per mesh on stderr, the count in
 *     GiCRenderStats.inactiveTriangleCount;
 *   - every triangle of an instance whose composed transform has a non-finite entry or no finite inverse (NaN, singular, zero matrix) is inactive;
 *   - giCCreateMaterial refuses a parameter block with a non-finite entry (NULL, like a material the reference fails to compile: the caller falls back to its default
 *     material); a light with a non-finite field is left out of the device arrays and the light counts until a setter repairs it (one warning on stderr);
 *   - a normal / tangent with a non-finite component is taken as +Z, a non-finite texture coordinate as 0, a non-finite bitangent sign as +1;
 *   - giCRender refuses (GI_C_ERROR, giCGetLastError names the field): a camera or dome light with a non-finite field, a forward / up vector that cannot be normalised, a vertical
 *     field of view outside (0, pi); non-finite float render settings (maxSampleValue may be +inf: no clamp); spp 0; mediumStackSize > 15; images beyond 65 535
 *     pixels a side (imageDims is packed 16 + 16 bits, rp_main.h:25-56).  A 0 x N image is a no-op (GI_C_OK).  spp x pixels may exceed 2^32: the frame is cut
 *     into batches of fewer than 2^32 work items.
 * Never a crash, a hang or a NaN pixel from geometry; every accepted case renders the image the oracle renders from the same scene with the inactive triangles
 * replaced by zero-area ones. */
int giCRender(const GiCRenderParams* params);

/* Gi.h:220-221 */
GiCScene* giCCreateScene(void);
void giCDestroyScene(GiCScene* scene);

/* Gi.h:223-228 */
GiCSphereLight* giCCreateSphereLight(GiCScene* scene);
void giCDestroySphereLight(GiCScene* scene, GiCSphereLight* light);
void giCSetSphereLightPosition(GiCSphereLight* light, const float* position);
void giCSetSphereLightBaseEmission(GiCSphereLight* light, const float* rgb);
void giCSetSphereLightRadius(GiCSphereLight* light, float radiusX, float radiusY, float radiusZ);
void giCSetSphereLightDiffuseSpecular(GiCSphereLight* light, float diffuse, float specular);

/* Gi.h:230-235 */
GiCDistantLight* giCCreateDistantLight(GiCScene* scene);
void giCDestroyDistantLight(GiCScene* scene, GiCDistantLight* light);
void giCSetDistantLightDirection(GiCDistantLight* light, const float* direction);
void giCSetDistantLightBaseEmission(GiCDistantLight* light, const float* rgb);
void giCSetDistantLightAngle(GiCDistantLight* light, float angle);
void giCSetDistantLightDiffuseSpecular(GiCDistantLight* light, float diffuse, float specular);

/* Gi.h:237-243 */
GiCRectLight* giCCreateRectLight(GiCScene* scene);
void giCDestroyRectLight(GiCScene* scene, GiCRectLight* light);
void giCSetRectLightOrigin(GiCRectLight* light, const float* origin);
void giCSetRectLightTangents(GiCRectLight* light, const float* t0, const float* t1);
void giCSetRectLightBaseEmission(GiCRectLight* light, const float* rgb);
void giCSetRectLightDimensions(GiCRectLight* light, float width, float height);
void giCSetRectLightDiffuseSpecular(GiCRectLight* light, float diffuse, float specular);

/* Gi.h:245-251 */
GiCDiskLight* giCCreateDiskLight(GiCScene* scene);
void giCDestroyDiskLight(GiCScene* scene, GiCDiskLight* light);
void giCSetDiskLightOrigin(GiCDiskLight* light, const float* origin);
void giCSetDiskLightTangents(GiCDiskLight* light, const float* t0, const float* t1);
void giCSetDiskLightBaseEmission(GiCDiskLight* light, const float* rgb);
void giCSetDiskLightRadius(GiCDiskLight* light, float radiusX, float radiusY);
void giCSetDiskLightDiffuseSpecular(GiCDiskLight* light, float diffuse, float specular);

/* Gi.h:253-257.  The dome light is an equirectangular image looked up by miss rays (rp_main.miss:46-86).  filePath is
 * decoded when it is a Radiance .hdr (RGBE), a .pfm, a .png or a baseline .jpg; other formats need imgio (out of scope) -- hand the decoded pixels
 * over with giCSetDomeLightTexture instead.  A dome light without an image is ignored, exactly like a dome light whose file
 * fails to load in the reference (Gi.cpp:2221-2230): miss rays then see the fallback dome (the colour clear value). */
GiCDomeLight* giCCreateDomeLight(GiCScene* scene, const char* filePath);
void giCSetDomeLightTexture(GiCDomeLight* light, GiCTexture* texture); /* [ext] */
void giCDestroyDomeLight(GiCDomeLight* light);
void giCSetDomeLightRotation(GiCDomeLight* light, const float* quat);
void giCSetDomeLightBaseEmission(GiCDomeLight* light, const float* rgb);
void giCSetDomeLightDiffuseSpecular(GiCDomeLight* light, float diffuse, float specular);

/* Gi.h:259-261 */
GiCRenderBuffer* giCCreateRenderBuffer(uint32_t width, uint32_t height, int32_t format /* GiCRenderBufferFormat */);
void giCDestroyRenderBuffer(GiCRenderBuffer* renderBuffer);
void* giCGetRenderBufferMem(GiCRenderBuffer* renderBuffer);

/* [ext] device-resident copy of the render buffer (valid after the first giCRender that bound it), so a
 * multi-GPU caller can gather tiles with RCCL without a host round trip. */
void* giCGetRenderBufferDeviceMem(GiCRenderBuffer* renderBuffer);
/* [ext] when nonzero, giCRender leaves results on the device only (no D2H copy); default 0 = reference behaviour */
void giCSetRenderBufferDeviceOnly(GiCRenderBuffer* renderBuffer, int32_t deviceOnly);
/* [ext] a render buffer that is host memory alone: no device copy, no HIP call, usable without giCInitialize.  It serves giCDenoise with
 * GI_C_DENOISE_SOURCE_HOST_FORM (every buffer) and as an INPUT of the other sources (sent from its memory); giCRender refuses it.  Destroyed with
 * giCDestroyRenderBuffer; giCGetRenderBufferDeviceMem answers NULL. */
GiCRenderBuffer* giCCreateHostRenderBuffer(uint32_t width, uint32_t height, int32_t format /* GiCRenderBufferFormat */);

/* [ext] Denoiser of the colour AOV: an edge-stopping a-trous wavelet filter guided by the normal, depth and (optionally) albedo AOVs the library already
 * renders -- what a viewport shows during the first seconds after an edit is a 1 - 16 spp image.  The filter is this library's own: nothing in the reference
 * pins it.  It is specified in DESIGN.md section 6 "Denoiser" and gi_denoise.h: `iterations` Jacobi passes of a 5 x 5 B3-spline kernel at steps 1, 2, 4 ...,
 * over colour / max(albedo, albedoFloor), with rational weights 1 / (1 + d^2) on depth (scale sigmaDepth; the depth AOV is log-depth) and on colour (scale
 * sigmaColor, halved every pass) and max(n_p . n_q, 0) squared `normalSquarings` times on the normals.  Pixels whose depth is `backgroundDepth` (exact
 * compare: bind the depth AOV with that clear value) or not finite, or whose colour or normal is not finite, are UNGUIDED: they come out bytewise as they
 * went in and contribute to no other pixel.  Alpha is passed through.  Only + - x / and a maximum on fp32 in one association: the device kernels
 * (gi_denoise.hip), the host form and tests/denoise_ref.py agree bit for bit.
 *
 * color / normal / albedo / output are Float32Vec4 buffers, depth a Float32 one, all of one size (sides at most 65535); albedo may be NULL.  Inputs are
 * never written -- giCRender's progressive accumulation reads the previous colour back from the colour buffer's device copy -- so `output` must be a buffer
 * of its own: aliasing an input is refused.
 *   GI_C_DENOISE_SOURCE_AUTO       an input is read from its DEVICE COPY when the last giCRender that bound it rendered the whole frame on the primary device
 *                                  alone; otherwise (a row share, a multi-device render, never rendered) it is sent from its host memory, and if it is
 *                                  deviceOnly the call is refused.
 *   GI_C_DENOISE_SOURCE_HOST       every input is sent from its host memory (tests feed synthetic guides).
 *   GI_C_DENOISE_SOURCE_HOST_FORM  the host form runs on the calling thread and touches no device; works without giCInitialize.  The result goes to `output`'s
 *                                  host memory alone.
 * AUTO and HOST launch on the primary device's stream without a host wait between passes, write `output`'s device copy, and copy it to `output`'s host memory
 * unless `output` is deviceOnly; they return when that is done.  Scratch (three Float32Vec4 planes, and a staging plane per sent input) belongs to the library,
 * is reused while the size does not change and freed by giCTerminate.
 * Refused with GI_C_ERROR and a giCGetLastError message: a NULL params or required buffer, sizes that differ, a wrong format, aliasing, iterations outside
 * 1 .. 6, normalSquarings above 6, a sigma or floor that is not finite or not positive, a non-finite backgroundDepth, an unknown source.
 * NOT concurrent with a giCRender that binds any of the buffers, nor with another giCDenoise on one of them (calls are serialised inside the library). */
#define GI_C_DENOISE_SOURCE_AUTO 0
#define GI_C_DENOISE_SOURCE_HOST 1
#define GI_C_DENOISE_SOURCE_HOST_FORM 2
typedef struct GiCDenoiseParams {
  GiCRenderBuffer *color, *albedo /* may be NULL */, *normal, *depth, *output;
  uint32_t iterations, normalSquarings;
  float sigmaColor, sigmaDepth, backgroundDepth, albedoFloor;
  int32_t source;   /* GI_C_DENOISE_SOURCE_* */
} GiCDenoiseParams;
/* of the last giCDenoise that ran in this process (a refused call leaves them alone) */
typedef struct GiCDenoiseStats {
  int32_t source;          /* what the call did: AUTO = every input read from its device copy, HOST = at least one input sent, HOST_FORM */
  uint32_t deviceInputs;   /* bit mask of the inputs read from their device copy: 1 colour, 2 normal, 4 depth, 8 albedo, 16 moments ...  */
  uint32_t sentInputs;     /* ... and of those sent from host memory                                                                     */
  uint32_t iterations;
  uint32_t width, height;
  uint64_t bytesSent;      /* host-to-device bytes of the sent inputs                                                                    */
  double prepareMs;        /* device events: k_denoise_prepare (HOST_FORM: host clock) ...                                               */
  double passMs[6];        /* ... each k_denoise_pass ...                                                                                */
  double copyMs;           /* ... and the copy of the output to host memory (0 for a deviceOnly output)                                  */
  double sendMs;           /* the host-to-device copies of the sent inputs                                                               */
  double totalMs;          /* host clock around the whole call                                                                           */
} GiCDenoiseStats;
void giCDenoiseDefaults(GiCDenoiseParams* params); /* iterations 5, normalSquarings 4, sigmaColor 2, sigmaDepth 0.02, backgroundDepth 1, albedoFloor 1e-3, AUTO; buffers NULL */
int giCDenoise(const GiCDenoiseParams* params);
int giCGetDenoiseStats(GiCDenoiseStats* out);

/* [ext] The variance-guided denoiser: giCDenoise with the colour weight's fixed sigma replaced, per pixel, by the variance of the pixel's mean, taken from a
 * sample-moments buffer (GI_C_AOV_EXT_MOMENTS) rendered beside the colour -- loose where a pixel is noisy, tight where it has converged, whatever the sample
 * count.  Specified in DESIGN.md section 6 "Denoiser" and gi_denoise.h: per pixel with n = M.z >= minSamples and finite sums, v = max(S2 / n - (S1 / n)^2, 0) /
 * (n - 1) / lum(max(albedo, albedoFloor))^2; per pass a guided pixel whose v is known weighs a tap's colour by 1 / (1 + dl^2 / (sigmaVariance^2 (vt +
 * varianceFloor))), dl the difference of the two luminances and vt the 3 x 3 {1/4, 1/2, 1/4}^2 average of v around the pixel, and v travels with the colour
 * (v' = sum w^2 v / (sum w)^2).  A pixel with fewer than minSamples samples, sums that are not finite or a v above 1e30 uses giCDenoise's weight with
 * base.sigmaColor.  Everything else -- the guides, the unguided pixels, the three sources, the scratch (two 8-byte planes more, allocated by the first call of
 * this entry), "inputs are never written", the refusals, giCGetDenoiseStats (prepareMs covers both prepare kernels; deviceInputs / sentInputs bit 16: the
 * moments) -- is giCDenoise's, and the same operator set in one association: the device kernels (gi_denoise_var.hip), the host form and
 * tests/denoise_var_ref.py agree bit for bit.  Refused in addition: a NULL moments buffer (giCDenoise is the fixed filter), one of another format or size or
 * that is the output, minSamples below 2, a sigmaVariance or varianceFloor that is not finite and positive. */
typedef struct GiCDenoiseVarianceParams {
  GiCDenoiseParams base;
  GiCRenderBuffer* moments;
  float sigmaVariance, varianceFloor;
  uint32_t minSamples;
} GiCDenoiseVarianceParams;
void giCDenoiseVarianceDefaults(GiCDenoiseVarianceParams* params); /* base: giCDenoiseDefaults; sigmaVariance 4, varianceFloor 1e-6, minSamples 2; moments NULL */
int giCDenoiseVariance(const GiCDenoiseVarianceParams* params);

/* [ext] statistics of the last giCRender on this scene; countTraversal != 0 in giCSetSceneOption enables
 * node/triangle counters (slower; measurement runs only). */
int giCGetRenderStats(const GiCScene* scene, GiCRenderStats* out);
#define GI_C_SCENE_OPTION_COUNT_TRAVERSAL 1
/* value N > 0: record HIP events around the stage launches of every N-th wavefront iteration (1 = every launch; events
 * on every launch cost ~16 % of a frame) and scale the per-stage totals accordingly; 0 = off */
#define GI_C_SCENE_OPTION_KERNEL_TIMERS 2
/* size of the persistent path pool (slots; default 4 Mi) and of the per-sample colour buffer (MiB; default 49152, at most a sixth of the device's memory) -- results
 * do not depend on either (tests/test_gpu_parity.py::test_pool_and_batch_invariance); 0 restores the default */
#define GI_C_SCENE_OPTION_POOL_SLOTS 3
#define GI_C_SCENE_OPTION_SAMPLE_BUFFER_MB 4
/* Refill threshold of k_trace_dyn, the traversal kernel for scenes beyond LDS and LDS-resident trees deeper than 8 levels: N in 1..64 = its persistent
 * waves claim new rays once N lanes are idle (default 8); -1 or 0 = default (0 is kept for existing callers).  The image does not depend on N. */
#define GI_C_SCENE_OPTION_TRACE_DYNAMIC 5
#define GI_C_SCENE_OPTION_TWO_LEVEL 6     /* [ext] 1: two-level BVH (TLAS over instances + one object-space BLAS per mesh) for scenes beyond LDS; default 0: one
                                             flat BVH over the instanced triangles (faster today); the image does not depend on it */
/* [ext] Scenes whose whole BVH fits LDS (<= 384 nodes, <= 128 triangles; no medium stack, no dome image) are rendered by a fused persistent kernel:
 * -1 (default), 1 or 2 = k_path, one path per lane in registers (1 and 2 are kept for existing callers); 0 = run the wavefront stage kernels on
 * them too.  The image does not depend on it. */
#define GI_C_SCENE_OPTION_FUSED_PATH 7
/* [ext] upper bound on the devices a giCRender of this scene uses (0 = all the library was initialised on; 1 = primary only). */
#define GI_C_SCENE_OPTION_DEVICES 8
/* [ext] who builds the flat BVH8: 0 (default) = the host builder; 1 = the device builder (Morton sort, PLOC, the same cost-optimal 8-wide collapse, written
 * straight into device memory).  It applies to scenes that take the flat layout and have more than 128 flattened triangles; every other
 * scene (the two-level layout, small LDS-resident scenes) keeps the host builder.  Out of device memory during the build falls back to the host builder.
 * GATLING_OPTIONS=device_build=0|1 overrides it.  The image does not depend on it. */
#define GI_C_SCENE_OPTION_BVH_BUILD 9
/* [ext] Sample look-ahead for progressive low-spp rendering (hdGatling's default frame is one sample per pixel and call): value N >= 2 = a giCRender call may trace
 * the samples of the next calls as well, in one batch (a "window" of at most N calls), keep them in the scene's per-sample buffer and serve each following call --
 * as long as nothing that enters an image has changed -- by folding ITS spp samples into the colour AOV without tracing a ray.  0 or 1 = off (default 0).
 * Windows ramp up 1, 2, 4 ... N calls after every reset of the accumulation, so an edit throws away fewer samples than were served since the previous one, and
 * never more than N - 1 calls' worth.  Every image of every call is the image the library returns without the option.  Look-ahead declines (the call renders as
 * without it) when progressiveAccumulation is off, a NEE / Bounces / ClockCycles AOV is bound, or the call itself needs more than one batch; the memory plan
 * (GI_C_SCENE_OPTION_SAMPLE_BUFFER_MB, free device memory) bounds the window.  Cost: the call that traces a window of K takes about K calls' samples at batch
 * rate and the K - 1 after it are short -- mean latency falls, per-call latency becomes uneven -- and the window holds pixels * K * spp * 16 bytes between
 * calls.  GATLING_OPTIONS=lookahead=N overrides it.  See giCGetLookaheadStats and the note below GiCRenderStats. */
#define GI_C_SCENE_OPTION_SAMPLE_LOOKAHEAD 10
/* [ext] Incremental visibility edits: value 1 = a giCSetMeshVisibility on a mesh of the built scene is applied to the device-resident scene by the next giCRender
 * -- the triangles behind the mesh in scene order are renumbered as a fresh build would number them, the mesh's own triangles stop being hit (or are hit
 * again) -- instead of rebuilding the scene; 0 = off (default): every visibility edit rebuilds, as in the reference (Gi.cpp:801-804).  The library falls
 * back to the rebuild when anything but visibility edits asked for one, when a toggled mesh is not part of the built scene (it was invisible at the build),
 * when fewer than 4096 visible flattened triangles remain, with GATLING_OPTIONS=incremental=0, and on the two-level layout.  After such an edit
 * GiCRenderStats.triangleCount and nodeCount keep describing what is RESIDENT on the device (hidden triangles included), bvhBuildMs is 0 and uploadMs the
 * time of the update.  Hidden geometry keeps its boxes in a flat tree until the next full build.  The image does not depend on the
 * option.  GATLING_OPTIONS=visibility_updates=0|1 overrides it (hdGatling sets no scene options). */
#define GI_C_SCENE_OPTION_VISIBILITY_UPDATES 11
/* [ext] Incremental vertex edits: value 1 = a giCSetMeshVertices on a mesh of the built scene is applied to the device-resident scene by the next giCRender --
 * the mesh's vertex and shading records are re-sent, its flattened triangles are made again and the scene BVH is REFITTED in device memory (same topology,
 * new conservative boxes; the partitioned layout refits the parts of the mesh and rebuilds its top tree) -- instead of rebuilding the scene; 0 = off
 * (default): a vertex edit rebuilds.  The image does not depend on the option (traversal contract: results do not depend on the tree).  The library falls
 * back to the rebuild when anything but vertex edits (and, with GI_C_SCENE_OPTION_VISIBILITY_UPDATES, visibility edits) asked for one, when an edited mesh is
 * not part of the built scene or is hidden by the visibility path, when a new position is not finite or beyond 1e18 (in object or world space), when the
 * scene had inactive triangles at its build, with fewer than 4096 resident triangles, with GATLING_OPTIONS=incremental=0, on the two-level layout and when
 * the device cannot hold the temporaries (32 bytes per node).  After such an edit GiCRenderStats.bvhBuildMs is 0 and uploadMs the time of the update.  A
 * refitted tree keeps the topology chosen for the OLD positions: large deformations make it slower to walk (never wrong); any full build resets that
 * (DESIGN.md section 6).  GATLING_OPTIONS=vertex_updates=0|1 overrides the option (hdGatling sets no scene options). */
#define GI_C_SCENE_OPTION_VERTEX_UPDATES 12
/* [ext] Incremental topology edits: value 1 = meshes created (giCCreateMesh and the setters that follow it) and destroyed (giCDestroyMesh) since the last
 * giCRender are applied to the device-resident scene -- a destroyed mesh of the built scene is taken out of the tree and the triangles behind it are
 * renumbered as a fresh build would number them; a new mesh gets its records at the ends of the device arrays and one subtree per instance under a rebuilt top
 * tree (built by the host, or on the device for parts of at least GATLING_OPTIONS=device_parts_min faces when GI_C_SCENE_OPTION_BVH_BUILD is 1) -- instead of
 * rebuilding the scene; 0 = off (default): every creation and destruction rebuilds.  This is what hdGatling does for every points, primvar or topology change
 * of a prim (destroy, create, every setter again).  With the option wanted giCDestroyMesh keeps a mesh of the built scene alive inside the library until the
 * next full build; the handle is invalid for the caller all the same.  The image does not depend on the option.  The library falls back to the rebuild when
 * anything else asked for one (instance counts or ids of a built mesh, scene options), with GATLING_OPTIONS=incremental=0, on the two-level layout, for a
 * scene within LDS, when fewer than 4096 visible flattened triangles remain, when a new mesh has a position that is not finite or beyond 1e18 (in object or
 * world space) or an unusable transform, when a new mesh lies in front of a mesh of the built scene in creation order (a mesh that was invisible or without a
 * valid material at the build and is now shown), when the top tree outgrows the range reserved for it, at 2^26 resident triangles, when the retired
 * triangles outnumber the live ones (resident memory stays within twice the live scene), when the first such edit of a scene destroys more of the built
 * triangles than it leaves, and when device memory runs out.  After such an edit
 * GiCRenderStats.triangleCount and nodeCount describe what is RESIDENT on the device (retired triangles and node reserves included), bvhBuildMs is the time
 * spent building the new subtrees and uploadMs the rest.  The first such edit of a scene re-lays it out as per-instance subtrees (about one build).
 * GATLING_OPTIONS=topology_updates=0|1 overrides the option (hdGatling sets no scene options).  DESIGN.md section 6. */
#define GI_C_SCENE_OPTION_TOPOLOGY_UPDATES 13
/* [ext] Resyncs as refits: value 1 = when GI_C_SCENE_OPTION_TOPOLOGY_UPDATES and GI_C_SCENE_OPTION_VERTEX_UPDATES are both wanted (the option is read only
 * then), a mesh destroyed and a mesh created since the last giCRender whose faces are the same -- hdGatling's answer to a points or primvar change of a prim
 * -- are recognised as ONE edited mesh: the new mesh ADOPTS the resident records of the destroyed one, nothing is retired and nothing is appended, and what
 * differs goes down the existing paths: new points refit the resident subtree (only if the vertex bytes differ), another material or other primvars take the
 * material update, other transforms the transform update; 0 = off (default): the pair is retired and appended.  A pair is adopted when the faces (count and
 * bytes), face ids, maxFaceId, vertex count, isLeftHanded, isDoubleSided, id, instance count and instance ids are equal; when the vertex update could refit
 * the destroyed mesh's records with the new points (it is not hidden by the visibility path, the positions are finite and within 1e18 in object and world
 * space, no triangle of its subtrees or of the scene was inactive at the build); and when no new mesh that is not itself adopted was created before it.
 * Meshes are paired in creation order, the first partner that qualifies wins.  Any other pair is retired and appended as without the option -- never
 * rebuilt for that reason.  The adopting mesh keeps its place in creation order: its triangles and those of the meshes behind the destroyed one get the ids a
 * fresh build gives them.  Resident triangle and node counts do not grow with such edits, so the rebuild that compacts retired triangles does not come due.
 * The image does not depend on the option.  GATLING_OPTIONS=resync_refits=0|1 overrides it (hdGatling sets no scene options).  DESIGN.md section 6. */
#define GI_C_SCENE_OPTION_RESYNC_REFITS 14
/* [ext] Incremental instancer edits: value 1 = when GI_C_SCENE_OPTION_TOPOLOGY_UPDATES is wanted (the option is read only then), giCSetMeshInstanceIds and a
 * giCSetMeshInstanceTransforms with another instance count on a mesh of the built scene -- what hdGatling sends for every DirtyInstancer / DirtyInstanceIndex
 * sync of a prim -- are applied to the resident scene by the topology update instead of rebuilding it; 0 = off (default): they rebuild.  New ids alone re-send
 * the mesh's instance records (equal ids send nothing).  A smaller count retires the instances behind the new count: their subtrees leave the top tree, their
 * records stay resident until the next build and count as retired triangles.  A larger count appends one instance record, one triangle range and one subtree
 * per new instance, built as the parts of a new mesh are; with GATLING_OPTIONS=instance_clone=1, where a live sibling instance of the mesh is resident with
 * a whole subtree, the new one is made from it in device memory instead (records and nodes copied, re-transformed and refitted: a cheaper edit, a tree that
 * costs more to walk).
 * The triangles behind get the ids a fresh build gives them; kept instances whose transform changed go through the transform update.  The image does not
 * depend on the option.  The scene is rebuilt instead for everything GI_C_SCENE_OPTION_TOPOLOGY_UPDATES rebuilds for, for a new count of 0 and for a mesh
 * hidden by the visibility path.  GATLING_OPTIONS=instance_updates=0|1 overrides it (hdGatling sets no scene options).  DESIGN.md section 6. */
#define GI_C_SCENE_OPTION_INSTANCE_UPDATES 15
/* [ext] Incremental transform edits on the two-level layout (GI_C_SCENE_OPTION_TWO_LEVEL, or chosen automatically from 2^26 flattened triangles): value 1 = a
 * giCSetMeshTransform, or a giCSetMeshInstanceTransforms with an unchanged instance count, on a mesh of a built two-level scene is applied to the resident
 * scene by the next giCRender when nothing else asks for a rebuild: the moved instances' records are re-sent, their world boxes are made on the device from
 * the mesh's BLAS triangles, the TLAS is built again on the host over the instance boxes and re-sent, and the flat tree that AOVs and giCTraceRays walk is
 * refitted in device memory; every BLAS stays.  0 = off (default): such an edit rebuilds the scene, as before.  The image does not depend on the option.
 * The scene is rebuilt instead when: there is no host copy of the scene or GATLING_OPTIONS=incremental=0; fewer than 4 096 triangles are resident; the
 * scene was built with inactive triangles; the flat tree has no level table (it was built on the device); a moved instance's transform is not finite or
 * not invertible, or carries a corner of its mesh beyond 1e18 (or to a non-finite value) in object or world space; the new TLAS would be too deep for the
 * layout's 16-entry stack (a fresh build would leave the two-level layout); the device has no memory for the refit's boxes (32 bytes per node).  A material
 * edit due in the same render is applied first, by the material update.  GATLING_OPTIONS=tlas_updates=0|1 overrides the option (hdGatling sets no scene
 * options).  DESIGN.md section 6. */
#define GI_C_SCENE_OPTION_TLAS_UPDATES 16
/* [ext] Incremental vertex edits on the two-level layout; read only when vertex updates are wanted (GI_C_SCENE_OPTION_VERTEX_UPDATES, or
 * GATLING_OPTIONS=vertex_updates=1): value 1 = a giCSetMeshVertices on a mesh of a built two-level scene is applied to the resident scene by the next
 * giCRender when nothing else asks for a rebuild: the mesh's vertex records are re-sent, its shading records and BLAS triangles are made again on the device,
 * its BLAS -- one per mesh, shared by all its instances -- keeps its topology and is refitted level by level in device memory, the world boxes of the mesh's
 * instances are made on the device, the TLAS is built again on the host over the instance boxes and re-sent, and the flat tree that AOVs and giCTraceRays
 * walk is refitted as well.  0 = off (default): such an edit rebuilds the scene, as before.  The image does not depend on the option; a refitted BLAS costs
 * more to walk the further its mesh deformed, until the next full build.  The scene is rebuilt instead when: there is no host copy of the scene or
 * GATLING_OPTIONS=incremental=0; fewer than 4 096 triangles are resident; the scene was built with inactive triangles; the flat tree has no level table (it
 * was built on the device); an edited mesh is not part of the built scene, is hidden or has another instance count; a new position is not finite or beyond
 * 1e18, or an instance of the mesh carries one beyond 1e18 in world space or has a transform that is not finite or not invertible; the new TLAS would be too
 * deep for the layout's 16-entry stack; the device has no memory for the refits' boxes (32 bytes per node).  A visibility toggle due in the same render
 * rebuilds on this layout.  GATLING_OPTIONS=blas_updates=0|1 overrides the option (hdGatling sets no scene options).  DESIGN.md section 6. */
#define GI_C_SCENE_OPTION_BLAS_UPDATES 17
/* [ext] Incremental visibility edits on the two-level layout; read only when visibility updates are wanted (GI_C_SCENE_OPTION_VISIBILITY_UPDATES, or
 * GATLING_OPTIONS=visibility_updates=1): value 1 = a giCSetMeshVisibility on a mesh of a built two-level scene is applied to the resident scene by the next
 * giCRender when nothing but visibility toggles asks for a rebuild: no BLAS, vertex, shading record or instance box changes; the scene-order ids of the
 * meshes behind a hidden one become a fresh build's in the flat records and in the per-instance traversal records, the table from such an id to its flat
 * record is made again in the same device pass, the flat records of a hidden mesh get zero edges (recomputed at the show), and the TLAS is built again on
 * the host over the boxes of the visible instances and re-sent.  0 = off (default): such an edit rebuilds the scene, as before.  The image does not depend
 * on the option; the flat tree that AOVs and giCTraceRays walk keeps the boxes of hidden geometry until the next full build.  The scene is rebuilt instead
 * when: there is no host copy of the scene or GATLING_OPTIONS=incremental=0; a toggled mesh has no records on the device (it was invisible or without a
 * valid material at the build); fewer than 4 096 triangles stay visible; the scene was built with inactive triangles; the new TLAS would be too deep for the
 * layout's 16-entry stack.  While a mesh is hidden, a transform or vertex edit OF THAT MESH rebuilds the scene (options 16 and 17 decline); edits of visible
 * meshes keep their paths and leave the hidden instances out of the TLAS.  A material edit due in the same render runs behind the visibility update, a
 * transform edit behind both; a vertex edit together with a toggle in one render rebuilds.  GATLING_OPTIONS=tlas_visibility=0|1 overrides the option
 * (hdGatling sets no scene options).  DESIGN.md section 6. */
#define GI_C_SCENE_OPTION_TLAS_VISIBILITY 18
/* [ext] Two-level scenes without the flat tree; read at the scene build, and only when the two-level layout is wanted (GI_C_SCENE_OPTION_TWO_LEVEL 1,
 * GATLING_OPTIONS=two_level=1, or 2^26 and more flattened triangles): value 1 = the flat BVH8 over all flattened triangles is neither built nor sent nor
 * kept -- the TLAS and the per-mesh BLASes are the scene's only trees.  The flat RECORDS stay, in scene order (the shading kernels read them); the non-colour
 * AOVs find their primary hits with a two-level walk (k_aov2), the scene bounds are the union of the instance boxes, and the edits in place of options 16,
 * 17 and 18 run without their flat refit.  0 = off (default): the flat tree is built beside the two-level arrays, as before.  The image does not depend on
 * the option.  The flat tree is built as before when: the scene has 128 triangles or fewer, or one inactive triangle (a vertex that is not finite or beyond
 * 1e18 after instancing), or the two-level layout declines (trees too deep for its 16-entry stack, 2^26 unique mesh triangles).  On a scene without the flat
 * tree GiCRenderStats.nodeCount is 0 and giCDebugValidateSceneBvh answers with an error.  GATLING_OPTIONS=tlas_only=0|1 overrides the option (hdGatling
 * sets no scene options).  DESIGN.md section 6. */
#define GI_C_SCENE_OPTION_TLAS_ONLY 19
/* [ext] Mesh creations and destructions on a two-level scene built without the flat tree (GI_C_SCENE_OPTION_TLAS_ONLY); read only with
 * GI_C_SCENE_OPTION_TOPOLOGY_UPDATES wanted (value 1 or GATLING_OPTIONS=topology_updates=1): value 1 = a giCDestroyMesh / giCCreateMesh of such a scene is
 * applied to the resident scene by the next giCRender when nothing else asks for a rebuild.  A destroyed mesh is retired as a visibility update hides one
 * (option 18's device pass renumbers the ids behind it; its instances leave the TLAS; its BLAS, flat records and shading records stay resident until the
 * next full build).  A created mesh is appended behind every built one: the host sends its vertex records, faces, face ids and instance records, builds its
 * one BLAS and the TLAS over one box more per instance; its shading records, BLAS triangles, flat records, face-id words and id-table words are made on
 * the device (gi_append.hip), so nothing per flattened triangle crosses the link.  0 = off (default): such an edit rebuilds the scene, as before.  The image
 * does not depend on the option.  The scene is rebuilt instead when: it keeps a flat tree (option 19 off, or declined at the build); there is no host copy or
 * GATLING_OPTIONS=incremental=0; fewer than 4 096 triangles stay visible; retired triangles outnumber live ones; a new mesh lies in front of a built one in
 * creation order; a new mesh has a vertex position that is not finite or beyond 1e18, an instance transform that is not finite or singular, or triangles
 * that leave the usable range in world space; the scene was built with inactive triangles; 2^26 unique BLAS triangles or 2^28 flat records would be
 * reached; the new TLAS would be too deep for the layout's 16-entry stack; a material index beyond 2^24; out of device memory; an instance count or id
 * edit of a built mesh is due and option 21 is not wanted.  Material, transform, vertex and visibility edits due in the same render take the paths of
 * options 16 - 18 behind this update.  GATLING_OPTIONS=tlas_topology=0|1 overrides the option (hdGatling sets no scene options).  DESIGN.md section 6. */
#define GI_C_SCENE_OPTION_TLAS_TOPOLOGY 20
/* [ext] Instancer edits -- giCSetMeshInstanceIds, giCSetMeshInstanceTransforms with another count -- on a mesh of a built two-level scene without the flat
 * tree; read only with options 13 (topology updates), 15 (instance updates) and 20 (two-level topology) wanted, on a scene built with option 19: value 1 =
 * the edit is applied to the resident scene by the next giCRender, with option 15's semantics.  Ids of kept instances are set in their records; a kept
 * instance that moved goes down option 16's path behind this update (without option 16 the scene is rebuilt); the instances [new, old) of a mesh that shrinks
 * retire -- out of the TLAS, their flat records made unhittable, the meshes behind renumbered by option 18's device pass -- and leave their storage slots on a
 * free list of the mesh; the instances [old, new) of a mesh that grows take free slots of the same mesh first, lowest first, then the ends of the arrays:
 * the host sends one instance record, one traversal record and one 32-byte job per new instance and builds the TLAS over all boxes; the flat records,
 * face-id words and id-table words of all new instances of all meshes are made on the device in one launch (gi_instances.hip).  The mesh's BLAS is shared and
 * not touched.  0 = off (default): such an edit rebuilds the scene, as before.  The image does not depend on the option.  The scene is rebuilt instead for
 * whatever option 20 declines for, a new count of 0, a mesh hidden by the visibility path, an unusable transform of a new instance, a move without option 16,
 * out of device memory.  GATLING_OPTIONS=tlas_instances=0|1 overrides the option (hdGatling sets no scene options).  DESIGN.md section 6. */
#define GI_C_SCENE_OPTION_TLAS_INSTANCES 21
/* [ext] Where the TLAS of an edit in place is built; read only where one of options 16, 17, 18, 20 or 21 applies an edit to a resident two-level scene: value
 * 1 = the TLAS over the instance boxes is built on the primary device (gi_tlas_build.hip: Morton sort, PLOC, a cost-optimal 8-wide collapse whose depth is
 * bounded by the layout's 16-entry stack, D = floor((15 - BLAS depth) / 2) levels) instead of by the host's binned-SAH builder; nodes and items are read back
 * and sent to every device as a host-built TLAS is.  0 = off (default): every launch, flag, counter and resident byte is what it is without the option.  The
 * image does not depend on the option (the traversal contract).  The host builder is used instead -- the edit never fails because of the option -- when the
 * scene has fewer instances than GATLING_OPTIONS=tlas_device_min (default in gi_options.h), when the tree does not fit D levels, out of device memory, or
 * on an error status; giCDebugSceneTlasBuildStats counts each.  The scene build itself keeps the host builder.  GATLING_OPTIONS=tlas_device_build=0|1
 * overrides the option (hdGatling sets no scene options); tlas_depth_budget=N lowers D for the device builder (tests).  DESIGN.md section 6. */
#define GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD 22
/* [ext] Where the BLAS of a mesh of a two-level scene is built; read where one is built: at the scene build, and where option 20 applies a mesh create to a
 * resident scene.  Value 1 = a mesh of at least GATLING_OPTIONS=blas_device_min and at most blas_device_max faces (defaults in gi_options.h) gets its BLAS
 * from the primary device (gi_blas_build.hip: padded face boxes from the uploaded points, then the stages of the device TLAS builder -- Morton sort, PLOC, a
 * cost-optimal 8-wide collapse whose depth is bounded by the layout's 16-entry stack, B = min(12, 15 - 2 * TLAS depth) levels) instead of from the host's
 * binned-SAH builder; nodes and face order are read back, and from there the host does what it does behind its own builder.  0 = off (default): every launch,
 * flag, counter and resident byte is what it is without the option.  The image does not depend on the option (the traversal contract).  The host builder is
 * used instead -- a build never fails because of the option -- for a mesh outside the face range, when the tree does not fit B levels, out of device memory,
 * or on an error status; giCDebugSceneBlasBuildStats counts each.  Vertex, visibility and instancer edits and option 22 compose unchanged on top of a
 * device-built BLAS.  GATLING_OPTIONS=blas_device_build=0|1 overrides the option (hdGatling sets no scene options); blas_depth_budget=N lowers B (tests).
 * DESIGN.md section 6. */
#define GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD 23
/* [ext] What becomes of the ranges options 20 and 21 retire -- the records of destroyed meshes, the storage slots of retired instances --; read only where
 * one of those options is about to apply an edit to a resident two-level scene without the flat tree.  Value 1 = before such an edit declines because
 * retired triangles outnumber live ones, the sync evaluates retired x 100 > live x P on the planned after-edit counts (P = GATLING_OPTIONS=
 * tlas_compact_percent, default 100: the point of that decline); where it holds and something retired by an EARLIER sync is resident, the scene is compacted
 * on the device first (gi_compact.hip): every mesh retired earlier and every free instance slot leaves every array, the live records move to the front of new
 * allocations in storage order with their indices rebased, the mesh records and scene-data tables are made again, the TLAS is built over the compacted
 * boxes.  The rule is then evaluated on the compacted scene and the edit goes on as without the option.  Live meshes, meshes hidden by option 18 and the
 * meshes the very same sync retires stay.  0 = off (default): every launch, flag, counter, statistic and resident byte is what it is without the option.  The
 * image does not depend on the option.  A compaction declines, leaving the scene untouched, for whatever option 20 declines for on the scene as it is, out of
 * device memory (new blocks are allocated on every device before anything resident changes), a TLAS over the compacted boxes that is too deep, or a count
 * that does not add up.  GATLING_OPTIONS=tlas_compaction=0|1 overrides the option (hdGatling sets no scene options).  DESIGN.md section 6. */
#define GI_C_SCENE_OPTION_TLAS_COMPACTION 24
/* [ext] Leaf lift; read at the scene build.  The flat tree of a scene the fused kernel walks out of LDS -- LDS-resident, not two-level, a root and one level
 * below it -- is handed to a pass (leaf_lift.cpp liftLeafSlots) that moves leaf slots of an internal child into free slots of the root while the builder's
 * cost model, evaluated over the dequantised slot boxes, strictly decreases: a leaf the top-down split left in a subtree it stretches is tested one level up,
 * and the child's box shrinks to the rest.  Internal topology and triangle ids are untouched; the image does not depend on the option (the traversal
 * contract).  -1 = the default (on), 0 = the builder's tree, byte for byte, 1 = on.  Setting it rebuilds the scene at the next render.
 * GATLING_OPTIONS=leaf_lift=0|1 overrides the option (hdGatling sets no scene options).  giCDebugSceneLeafLift reports what the last build moved.
 * DESIGN.md sections 1 and 6. */
#define GI_C_SCENE_OPTION_LEAF_LIFT 25
int giCGetLookaheadStats(const GiCScene* scene, GiCLookaheadStats* out);
int giCSetSceneOption(GiCScene* scene, int32_t option, int32_t value);
/* [ext] closest hit of one ray through the device traversal kernel (parity tests of the BVH8 path).
 * Returns 1 on hit (t,u,v, instance, prim written), 0 on miss, <0 on error.  Candidates on cut-out materials pass the any-hit test of the render
 * (rp_main.ahit:51-60) with the random state 0: the answer is a function of the ray and the scene alone. */
int giCTraceRays(GiCScene* scene, uint32_t count, const float* origins /*3*count*/, const float* dirs /*3*count*/,
                 float tMin, float tMax, float* outTUV /*3*count*/, int32_t* outInstPrim /*2*count, -1 on miss*/);

/* [ext] host-only self check of the BVH8 builder (no device needed): builds the tree over `triCount` triangles
 * (9 floats each: v0, v1, v2) and verifies that every triangle is reachable and lies inside the dequantised box of
 * every ancestor slot.  Returns the number of violations (0 = conservative), <0 on error. */
/* [ext] device-side known-answer hook: closed-form BSDF sample + evaluate for `count` explicit shading frames.
 * in: 22 floats per item (normal, tangentU, tangentV, geomNormal, k1, k2, xi[4]); out: 15 floats per item
 * (k2, bsdf_over_pdf, pdf, event, eval diffuse, eval glossy, eval pdf). */
int giCDebugEvalBsdf(const GiCMaterialDesc* desc, uint32_t count, const float* in, float* out);
/* [ext] host-only: the shade class an untextured material's hits are binned and shaded by (k_shade variants; the reference compiles one hit shader per material with
 * feature #defines, GlslShaderGen.cpp:204-274): 0 diffuse, 1 UsdPreviewSurface, 2 OpenPBR with every lobe, 3 OpenPBR BASE (no coat / fuzz / thin film / anisotropy /
 * transmission / subsurface, not thin-walled, all parameters finite).  giCDebugEvalBsdf runs the variant this names.  <0 on error. */
int giCDebugShadeClass(const GiCMaterialDesc* desc);
/* [ext] device self check: the kernels' square root (the compiler's correctly rounded expansion without the steps that ordinary arguments do not need) against sqrtf
 * for the `count` float bit patterns from `first` on; count = 2^32 covers every float.  Returns the number of arguments whose results differ (0), -1 on error. */
int64_t giCDebugCheckSqrt(uint32_t first, uint64_t count);
/* [ext] device self check: the fused kernels' division (the compiler's correctly rounded expansion without the steps that ordinary operands do not need; one
 * reciprocal for the three quotients of a vector by a scalar) against `/`.  mode 0: `count` pairs (numerator, denominator) of float bit patterns in `words`;
 * mode 1: `count` pairs drawn on the device from `seed`, every bit pattern equally likely (`words` unused); mode 2: `count` items (x, y, z, s) in `words`, checking
 * normalize(x, y, z) and (x, y, z) / s; mode 3: such items drawn on the device from `seed`, with zero and denormal components among ordinary ones; mode 4: the
 * reciprocal (1 / d in one correction step less) and 1 / sqrt(d) of the `count` bit patterns from `seed` on, count = 2^32 covers every float.  Modes 0 and 1 check 1 / d as well.
 * Returns the number of items with a result that differs in a bit (NaN equals NaN), -1 on error. */
int64_t giCDebugCheckDiv(uint32_t mode, uint64_t count, uint32_t seed, const uint32_t* words);
/* [ext] device-side hook for the MDL renderer runtime's remaining texture entry points (mdl_interface.glsl:45-65, 86-105, 167-221), which only MDL-generated code
 * calls: `rgba` = width x height x depth RGBA float texels (slice by slice; depth 1 = a 2-D image); per query 8 floats (kind, valid, c0, c1, c2, wrapU, wrapV, wrapW)
 * with kind 0 tex_texel_float4_2d(c0, c1), 1 tex_resolution_2d, 2 tex_lookup_float4_3d(c0, c1, c2; wraps), 3 tex_texel_float4_3d(c0, c1, c2); valid 0 = the invalid
 * texture; per result 4 floats. */
int giCDebugTexRuntime(const float* rgba, uint32_t width, uint32_t height, uint32_t depth, uint32_t count, const float* queries, float* out);
int giCDebugValidateBvh(const float* triVerts, uint32_t triCount, uint32_t* outNodeCount, uint32_t* outMaxDepth);
/* [ext] host-only walk for designing test scenes: builds the BVH8 over the `triCount` triangles of `triVerts` (9 floats each) as giCDebugValidateBvh does and runs
 * the traversal kernels' ordered walk (a node's hit internal children in octant-flipped slot order, nearest first, the rest pushed) for `rayCount` rays
 * (origins / dirs: 3 floats each), boxes only.  out[0] = levels of the tree, out[1] = nodes, out[2 + i] = the most stack entries the walk of ray i holds.
 * Nothing is culled -- no triangle is tested, every internal child whose box the ray meets counts --, so out[2 + i] is an UPPER BOUND on what a device walk of
 * that ray holds (exact for a ray that hits no triangle); the proof that a render filled a stack is giCDebugTraversalStackHigh.  Returns 0, <0 on error. */
int giCDebugBvhStackReach(const float* triVerts, uint32_t triCount, const float* origins, const float* dirs, uint32_t rayCount, uint32_t* out /* 2 + rayCount */);
/* [ext] the same host-only check for the partitioned layout incremental transform updates use: `partCount` consecutive triangle ranges, one
 * subtree each, joined by a top tree over the subtree roots.  Returns the violations of the assembled tree (0 = every triangle reachable and inside every
 * ancestor slot's box), <0 on error. */
int giCDebugValidatePartitionedBvh(const float* triVerts, uint32_t triCount, uint32_t partCount, uint32_t* outNodeCount, uint32_t* outMaxDepth);
/* [ext] host-only check of the BVH refit (gi_refit.h, the arithmetic the device kernels run): builds the tree over the `triCount` triangles of `triVertsA`
 * (9 floats each), moves them to `triVertsB`, refits the tree -- same topology, new boxes -- and validates it against B as giCDebugValidateBvh does.  Returns
 * the number of violations (0 = conservative), <0 on error; outNodeCount / outMaxDepth describe the tree, which a refit does not change. */
int giCDebugRefitBvh(const float* triVertsA, const float* triVertsB, uint32_t triCount, uint32_t* outNodeCount, uint32_t* outMaxDepth);
/* [ext] the nodes and triangles resident on device `deviceIndex` of a scene rendered at least once are downloaded and the host runs the refit over a copy of
 * them.  A refit is a function of the topology and the triangles alone, so the host must reproduce the resident bytes: returns the number of nodes whose 80
 * bytes differ (0 after a build as after a vertex update), <0 on error.  outNodes: nodes compared (partitioned layout: the parts' live nodes -- the top tree is
 * built over padded part bounds, not refitted). */
int giCDebugSceneRefitCheck(const GiCScene* scene, uint32_t deviceIndex, uint32_t* outNodes);
/* [ext] the tree resident on device `deviceIndex` (0 = primary) of a scene rendered at least once, downloaded and checked: every active triangle reachable and
 * inside every ancestor slot's box; and (flat, unpartitioned layout) nodes breadth-first, internal children contiguous in slot order at childBase, leaf
 * triangles contiguous at triBase, every active id once in [0, activeTris), the inactive ones behind in id order; depth <= 49.  outBuiltOnDevice: 1 when the
 * device builder made it; outDigest: a 64-bit hash of the node and triangle bytes.  Returns the number of violations, <0 on error. */
int giCDebugValidateSceneBvh(const GiCScene* scene, uint32_t deviceIndex, uint32_t* outNodeCount, uint32_t* outMaxDepth, int32_t* outBuiltOnDevice,
                             uint64_t* outDigest);

/* [ext] host-only: the dirty flags ONE edit raises on a scratch scene (one texture, two materials, one mesh; no device is touched), before the scene's first build
 * (`built` = 0) or after it (`built` = 1).  Flags: 1 full rebuild, 2 framebuffer reset, 4 lights, 8 materials, 16 transforms; materials or transforms WITHOUT
 * the rebuild bit take the incremental paths (see giCSetMeshMaterial).  `edit`: 0 giCCreateMaterial, 1 giCDestroyMaterial, 2 giCSetMeshMaterial,
 * 3 giCSetMaterialPrimvarInput, 4 giCSetMaterialTexture, 5 giCSetMaterialTextureTransform, 6 giCCreateTexture, 7 giCDestroyTexture, 8 giCSetMeshPrimvars,
 * 9 giCSetMeshInstancerPrimvars, 10 giCSetMeshTransform, 11 giCSetMeshVisibility, 12 giCSetMeshInstanceIds, 13 giCCreateMesh, 14 giCDestroyMesh,
 * 15 giCSetMeshInstanceTransforms with another instance count, 16 giCSetMeshVertices.  <0 on error. */
int32_t giCDebugEditDirtyFlags(int32_t edit, int32_t built);
/* [ext] how often the scene's geometry was brought up to date by outCounts[0] a full build, [1] an incremental transform update, [2] an incremental material
 * update, since the scene was created. */
int giCDebugSceneUpdateCounts(const GiCScene* scene, uint64_t* outCounts /* 3 */);
/* [ext] how often the scene was brought up to date by an incremental visibility update (GI_C_SCENE_OPTION_VISIBILITY_UPDATES); such an update is not counted
 * in giCDebugSceneUpdateCounts. */
int giCDebugSceneVisibilityUpdateCount(const GiCScene* scene, uint64_t* outCount);
/* [ext] how often the scene was brought up to date by an incremental vertex update (GI_C_SCENE_OPTION_VERTEX_UPDATES); not counted in
 * giCDebugSceneUpdateCounts either. */
int giCDebugSceneVertexUpdateCount(const GiCScene* scene, uint64_t* outCount);
/* [ext] [debug] how often the scene was brought up to date by an incremental topology update (GI_C_SCENE_OPTION_TOPOLOGY_UPDATES); not counted in
 * giCDebugSceneUpdateCounts either. */
int giCDebugSceneTopologyUpdateCount(const GiCScene* scene, uint64_t* outCount);
/* [ext] [debug] how many meshes adopted the resident records of the mesh they replaced (GI_C_SCENE_OPTION_RESYNC_REFITS) since the scene was created.  An update
 * that only adopts is counted as one topology update. */
int giCDebugSceneResyncCount(const GiCScene* scene, uint64_t* outCount);
/* [ext] [debug] host-only check that the shading records a vertex update GATHERS from the packed vertex records (gi_refit.h refit_gather_shade, the function the
 * device kernel k_gather_shade runs) are the records the scene build packs: both made for the mesh (`vertices`, `faces`: 3 indices per face), compared
 * bytewise.  Returns the number of records whose 160 bytes differ (0 is the contract), <0 on error (a null array, an index outside the vertices). */
int giCDebugGatherShade(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount);
/* [ext] [debug] what GI_C_SCENE_OPTION_INSTANCE_UPDATES did since the scene was created: out[0] scene syncs that applied an instancer edit in place, [1] instances
 * appended, [2] of those, made from a resident sibling instance on the device (gi_patch.hip k_clone_parts), [3] instances retired.  Such a sync is counted as
 * one topology update. */
int giCDebugSceneInstanceUpdateCount(const GiCScene* scene, uint64_t* out /* 4 */);
/* [ext] [debug] host-only check of the per-record arithmetic that makes a new instance from a resident sibling (gi_refit.h refit_clone_record, what k_clone_parts
 * runs): the mesh is flattened under the instance transform `xformA` (16 floats, USD row vectors) with the scene build's code, every record is cloned to the
 * instance transform `xformB` under another instance index and id base, and the result is compared bytewise with the scene build's records for `xformB`.
 * Returns the number of records whose 64 bytes differ (0 is the contract), <0 on error (a null array, an index outside the vertices, an unusable transform). */
int giCDebugCloneInstance(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, int32_t isLeftHanded, const float* xformA,
                          const float* xformB);
/* [ext] [debug] the vertex and shading records resident on device `deviceIndex` of a scene rendered at least once, downloaded and compared with the host's copies
 * over the WHOLE arrays (a store outside an edited range is seen).  Returns the number of shading records whose 160 bytes differ plus the vertex records
 * whose 48 bytes differ (0), <0 on error; outRecords: shading records compared (0 for a scene within LDS, which keeps none). */
int giCDebugSceneShadeCheck(const GiCScene* scene, uint32_t deviceIndex, uint32_t* outRecords);
/* [ext] [debug] how often the scene was brought up to date by a transform update of the two-level layout (GI_C_SCENE_OPTION_TLAS_UPDATES); not counted in
 * giCDebugSceneUpdateCounts either. */
int giCDebugSceneTlasUpdateCount(const GiCScene* scene, uint64_t* outCount);
/* [ext] [debug] the two-level arrays resident on device `deviceIndex` of a scene rendered at least once -- TLAS nodes, TLAS items, per-instance traversal
 * records, BLAS nodes, BLAS triangles -- downloaded and compared with the arrays the scene build's own code makes anew from the scene's current meshes.
 * Returns the number of records that differ bytewise (0 after a build as after every update in place), <0 on error.  After topology updates in place
 * (GI_C_SCENE_OPTION_TLAS_TOPOLOGY) the arrays are made anew over the meshes in storage order, appended ones at the end: every BLAS range is compared where it
 * lies; a retired (destroyed) mesh is a hidden one -- out of the TLAS -- and its BLAS ranges and traversal records are ignored; so is the storage slot a
 * retired instance left (GI_C_SCENE_OPTION_TLAS_INSTANCES) until a grow of its mesh takes it: the arrays are made over the live instances where they lie.  out[0]: 1 when the two-level layout is
 * in use (0: nothing was compared), [1] instances, [2] TLAS nodes, [3] TLAS depth. */
int giCDebugSceneTlasCheck(const GiCScene* scene, uint32_t deviceIndex, uint32_t* out /* 4 */);
/* (With GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD the check keeps its meaning, "what the scene's own code makes anew": the comparison TLAS is made by the builder
 * that made the resident one -- after an edit whose TLAS the device built, the host form of that builder (giCDebugBuildTlasHost's) over the same masked boxes
 * under the same depth budget -- so it still answers 0; the BLAS and traversal-record parts are unchanged, and so is everything with the option off.) */
/* [ext] [debug] the host form of the device TLAS builder (gi_tlas_build_host.cpp; no device is used): a TLAS over `count` boxes (6 floats each: min xyz, max
 * xyz; taken as they are) with at most `depthBudget` levels (clamped to 7) and PLOC radius `radius`, validated: every active item exactly once in items[0,
 * active), the inactive ones (an inverted box, a non-finite side, a magnitude beyond 1e18) behind in input order; nodes breadth-first, internal children
 * contiguous at childBase in slot order; every item box inside every ancestor slot's dequantised box; depth <= budget.  Returns the number of violations
 * (0), GI_C_TLAS_BUILD_TOO_DEEP when the tree cannot fit the budget, -1 on error.  out[0] nodes, [1] depth, [2] PLOC passes, [3] the tree's SAH model cost
 * (root area + per internal slot its area + per leaf slot 0.5 * items * its area, over the dequantised slot boxes), [4] the same function over
 * buildBvh8Boxes's tree of the same boxes, [5] host waits (0 here), [6] buildBvh8Boxes's depth, [7] active items. */
#define GI_C_TLAS_BUILD_TOO_DEEP (-2)
int giCDebugBuildTlasHost(const float* boxes6, uint32_t count, uint32_t depthBudget, uint32_t radius, double* out /* 8 */);
/* [ext] [debug] the device builder (gi_tlas_build.hip) on the same arguments: the same validation plus the node and item records that differ bytewise from the
 * host form's (0 is the contract); GI_C_TLAS_BUILD_TOO_DEEP exactly where the host form answers it.  out as above, [5] = waits of the host on the device
 * inside the build (bounded whatever `count`: gi_tlas_build.h kTlasMaxHostWaits). */
int giCDebugBuildTlas(const float* boxes6, uint32_t count, uint32_t depthBudget, uint32_t radius, double* out /* 8 */);
/* [ext] [debug] GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD on this scene: out[0] TLAS builds on the device, fallbacks to the host builder: [1] too deep, [2] out of
 * memory, [3] error status, [4] fewer instances than tlas_device_min; of the last device build: [5] - [8] stage times in microseconds (upload + boxes + sort,
 * PLOC, emission, read-back), [9] PLOC passes, [10] host waits, [11] depth, [12] nodes, [13] workspace allocations since the scene was created, [14] 1 when
 * the resident TLAS was made by the device builder, [15] the depth budget of that build.  All zero with the option off. */
int giCDebugSceneTlasBuildStats(const GiCScene* scene, uint64_t out[16]);
/* [ext] [debug] the host form of the BLAS builder of GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD (gi_blas_build_host.cpp) over one mesh, `depthBudget` levels at most (the
 * builder's own bound is 12), PLOC search radius `radius`.  Host only.  Returns the number of violated rules (0 is the contract: out[8] + out[9] + out[10] +
 * out[11] + out[13], + 1 where out[12] > 0), GI_C_TLAS_BUILD_TOO_DEEP when the tree cannot fit the budget, -1 on error (a face index outside the vertices is
 * one).  out[0] nodes, [1] depth, [2] PLOC passes, [3] the tree's SAH model cost (as giCDebugBuildTlasHost), [4] the same function over the host builder's
 * tree (buildMeshBlas), [5] host waits (0 here), [6] the host builder's depth, [7] active faces, [8] blasConservativeViolations of the tree over the mesh's
 * records, [9] rule violations of the tree over the padded face boxes (depth within the budget, every usable face named once, unusable faces behind in input
 * order, children behind parents breadth-first, every face inside every ancestor slot), [10] inconsistencies of the level table, [11] bytes of mlo / mhi that
 * differ from buildMeshBlas's, [12] with depthBudget <= 7: node and item records that differ from the TLAS builder's host form over the same boxes (else 0),
 * [13] node bytes a BLAS refit over the unchanged points changes (gi_blas.h blasRefitHost), [14] the depth budget the build ran under. */
int giCDebugBuildBlasHost(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, uint32_t depthBudget, uint32_t radius,
                          double* out /* 16 */);
/* [ext] [debug] the device builder (gi_blas_build.hip) on the same arguments: the number of node / order / mlo / mhi BYTES that differ from the host form's plus
 * the violated rules above, counted on the device's bytes (0 is the contract); GI_C_TLAS_BUILD_TOO_DEEP exactly where the host form answers it (when both say
 * so).  out as above, [5] = waits of the host on the device inside the build (bounded whatever faceCount: gi_tlas_build.h kTlasMaxHostWaits), [15] = the
 * differing bytes alone. */
int giCDebugBuildBlas(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, uint32_t depthBudget, uint32_t radius,
                      double* out /* 16 */);
/* [ext] [debug] GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD on this scene: out[0] BLAS builds on the device, fallbacks to the host builder: [1] fewer faces than
 * blas_device_min, [2] more than blas_device_max, [3] too deep, [4] out of memory, [5] error status; of the last device build: [6] - [9] stage times in
 * microseconds (upload + face boxes + sort, PLOC, emission, read-back), [10] PLOC passes, [11] host waits, [12] depth, [13] nodes, [14] its depth budget;
 * [15] meshes of the resident scene whose BLAS the device built.  All zero with the option off. */
int giCDebugSceneBlasBuildStats(const GiCScene* scene, uint64_t out[16]);
/* [ext] [debug] device check of the kernels that make the world boxes of moved instances (gi_tlas.hip k_inst_bounds / k_inst_finish): the mesh (`vertices`,
 * `faces`: 3 indices per face) under each of the `xformCount` instance transforms (16 floats each, USD row vectors).  outBoxes6 (6 floats per transform: min
 * xyz, max xyz, padded) and outStatus (one word per transform, 0 = usable; bits: 1 a corner unusable in object space, 2 in world space, 4 a flattened
 * triangle the builders would leave out) receive the device's results; either may be null.  Returns the number of (box, status) pairs that differ bytewise
 * from the host form of the same arithmetic (0 is the contract), <0 on error (no device, a null array, an index outside the vertices). */
int giCDebugInstanceBounds(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, const float* xforms16, uint32_t xformCount,
                           float* outBoxes6, uint32_t* outStatus);
/* [ext] [debug] how often the scene was brought up to date by a vertex update of the two-level layout (GI_C_SCENE_OPTION_BLAS_UPDATES); counted neither in
 * giCDebugSceneUpdateCounts nor in giCDebugSceneVertexUpdateCount. */
int giCDebugSceneBlasUpdateCount(const GiCScene* scene, uint64_t* outCount);
/* [ext] [debug] the two-level arrays resident on device `deviceIndex` of a scene rendered at least once, checked against the scene's current meshes after
 * vertex updates in place.  Counted as differences: (a) a resident BLAS triangle that does not carry the build's `prim` at its place or, bytewise, the
 * current corners of that face; (b) a resident BLAS node whose 80 bytes differ from the host form of the BLAS refit (gi_blas.h, children before parents) run
 * over the host's copy of the build's topology and the current points; (d) a resident TLAS node or item that differs bytewise from a fresh build's over the
 * current meshes (instance boxes do not depend on a BLAS's shape); (e) a resident per-instance traversal record that differs from the fresh one with its
 * BLAS root replaced by the resident BLAS's.  (c), reported separately: out[2] counts the violations of the conservative check -- every node's dequantised
 * slot box contains the padded boxes of all faces below it, every usable face is named by exactly one leaf slot.  A mesh retired by a topology update in place
 * (GI_C_SCENE_OPTION_TLAS_TOPOLOGY) is skipped: its ranges and records are ignored, as a hidden mesh it is out of the TLAS; the traversal record of a storage slot a
 * retired instance left (GI_C_SCENE_OPTION_TLAS_INSTANCES) is ignored likewise.  Returns the number of differences plus those violations (0), <0
 * on error.  out[0]: 1 when the two-level layout is in use (0: nothing was compared), [1] BLAS nodes compared, [2] conservative violations, [3] BLAS
 * triangles compared. */
int giCDebugSceneBlasCheck(const GiCScene* scene, uint32_t deviceIndex, uint32_t* out /* 4 */);
/* [ext] [debug] device check of the BLAS refit kernels (gi_blas.hip k_blas_tris / k_blas_refit_level): one BLAS is built on the host over the mesh with
 * points `a` (`faces`: 3 indices per face) as the scene build does, uploaded, and brought to points `b` by the kernels; the host form of the same arithmetic
 * (gi_blas.h) does the same.  Returns the number of node and triangle-record bytes that differ between device and host (0 is the contract) -- with a == b
 * (the same array, or the same positions) plus the bytes that differ from the build's --, <0 on error (no device, a null array, an index outside the
 * vertices).  outNodes: nodes of the BLAS; outViolations: violations of the conservative check over the device's result. */
int giCDebugBlasRefit(const GiCVertex* a, const GiCVertex* b, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, uint32_t* outNodes,
                      uint32_t* outViolations);
/* [ext] [debug] the host-only sibling: the host form of the BLAS refit alone, no device use.  Returns the number of bytes by which the refitted topology
 * (imask, meta, childBase, triBase of every node; prim of every record) differs from the build's -- with the same positions in a and b, the number of node
 * and record bytes that differ from the build's at all -- (0), <0 on error.  outNodes / outViolations as above. */
int giCDebugBlasRefitHost(const GiCVertex* a, const GiCVertex* b, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, uint32_t* outNodes,
                          uint32_t* outViolations);
/* [ext] [debug] how often the scene was brought up to date by a visibility update of the two-level layout (GI_C_SCENE_OPTION_TLAS_VISIBILITY); counted neither
 * in giCDebugSceneUpdateCounts nor in giCDebugSceneVisibilityUpdateCount. */
int giCDebugSceneTlasVisibilityUpdateCount(const GiCScene* scene, uint64_t* outCount);
/* [ext] [debug] how often the scene was brought up to date by a topology update of the two-level layout (GI_C_SCENE_OPTION_TLAS_TOPOLOGY); counted neither in
 * giCDebugSceneUpdateCounts nor in giCDebugSceneTopologyUpdateCount. */
int giCDebugSceneTlasTopologyUpdateCount(const GiCScene* scene, uint64_t* outCount);
/* [ext] [debug] device check of the kernels that make an appended mesh's records (gi_append.hip k_append_shade_index, k_append_blas_tris, k_append_records,
 * with gi_refit.hip k_gather_shade between them): the mesh (`vertices`, `faces`: 3 indices per face, `faceIds`: faceCount entries or NULL, `maxFaceId`,
 * `flags`: bit 0 flip-facing, bit 1 double-sided) under `xformCount` instance transforms (16 floats each, USD row vectors), laid out behind `vertexOffset`
 * vertex records, `shadeBase` shading records and the scene-order id `idBase`, with the word `matFlags`.  The kernels run on scratch arrays; returns the number
 * of BYTES of the shading records, BLAS records (in the host builder's order), flat records, face-id words and id-table words that differ from the scene
 * build's own host forms (flattenInstance, packTriShade, makeBlasTri, faceIdAovOf, id == position in the table) (0 is the contract), <0 on error (no device,
 * a null array, an index outside the vertices, an unusable transform).  giCDebugAppendRecordsHost: the host forms of the same kernels (gi_append.h) against
 * the same references; no device use. */
int giCDebugAppendRecords(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, const int32_t* faceIds, uint32_t maxFaceId,
                          uint32_t flags, const float* xforms16, uint32_t xformCount, uint32_t vertexOffset, uint32_t shadeBase, uint32_t idBase, uint32_t matFlags);
int giCDebugAppendRecordsHost(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, const int32_t* faceIds, uint32_t maxFaceId,
                              uint32_t flags, const float* xforms16, uint32_t xformCount, uint32_t vertexOffset, uint32_t shadeBase, uint32_t idBase,
                              uint32_t matFlags);
/* [ext] [debug] device check of the kernel that makes the flat records of new instances of built meshes (gi_instances.hip k_instance_records): `meshCount`
 * meshes (`flags`: bit 0 flip-facing, bit 1 double-sided; `faceIds`: faceCount entries or NULL) and `jobCount` new instances, each of mesh `mesh` under
 * `transform` (16 floats, USD row vectors), with the instance record `instanceSlot`, the flat records [recordSlot, recordSlot + the mesh's faces) and the
 * scene-order ids from `idBase` on -- slots in any order, with gaps.  ONE launch runs over scratch arrays pre-filled with a pattern; returns the number of
 * BYTES of the flat records, face-id words and id-table words that differ from the scene build's own host forms (flattenInstance, faceIdAovOf, id ==
 * position in the table), words outside every job's range included (0 is the contract), <0 on error (no device, a null array, an index outside the
 * vertices, an unusable transform, overlapping slots).  giCDebugInstanceRecordsHost: the host form of the same kernel (gi_instances.h) against the same
 * references; no device use. */
typedef struct GiCDebugInstanceMesh { const GiCVertex* vertices; const GiCFace* faces; const int32_t* faceIds; uint32_t vertexCount, faceCount, maxFaceId, flags; } GiCDebugInstanceMesh;
typedef struct GiCDebugInstanceJob { uint32_t mesh, instanceSlot, recordSlot, idBase; float transform[16]; } GiCDebugInstanceJob;
int giCDebugInstanceRecords(const GiCDebugInstanceMesh* meshes, uint32_t meshCount, const GiCDebugInstanceJob* jobs, uint32_t jobCount);
int giCDebugInstanceRecordsHost(const GiCDebugInstanceMesh* meshes, uint32_t meshCount, const GiCDebugInstanceJob* jobs, uint32_t jobCount);
/* [ext] [debug] instancer edits applied in place on the two-level layout (GI_C_SCENE_OPTION_TLAS_INSTANCES): out[0] = syncs applied, out[1] = instances
 * appended, out[2] = of those, how many went into reused storage slots, out[3] = instances retired.  Such a sync counts once in
 * giCDebugSceneTlasTopologyUpdateCount, and neither in giCDebugSceneUpdateCounts nor in giCDebugSceneInstanceUpdateCount. */
int giCDebugSceneTlasInstanceUpdateStats(const GiCScene* scene, uint64_t out[4]);
/* [ext] [debug] compactions of the retired ranges of this scene (GI_C_SCENE_OPTION_TLAS_COMPACTION): out[0] = compactions applied, out[1] = records moved
 * (items of all eight array kinds), out[2] = bytes of device memory released on the primary device (old blocks minus new ones), out[3] = compactions that
 * were due and declined.  A compaction is part of the sync that triggers it and has no entry in giCDebugSceneUpdateCounts. */
int giCDebugSceneCompactionCount(const GiCScene* scene, uint64_t out[4]);
/* [ext] [debug] device check of the kernel that compacts one array kind (gi_compact.hip k_compact_ranges).  `kind`: 0 FVertex, 1 BlasTri, 2 face-id words,
 * 3 TriShade, 4 Node8, 5 InstanceRec, 6 InstTrav, 7 TriRec; `records`: recordCount records of that kind; `ranges`: consecutive ranges that cover them in
 * order (their counts add up to recordCount; a count may be 0), each live or dead, a live one with the deltas its records' indices move by (by kind:
 * gi_compact.h) and, for kind 7, `hidden` != 0 where its records must not write the id table.  ONE launch moves all live ranges to the front of a scratch
 * array pre-filled with a pattern; for kind 7 an id table of one word per live record is pre-filled likewise.  Returns the number of BYTES of the new array
 * and the table that differ from a straightforward restatement -- the records of the live ranges filtered in order, then their fields rebased one by one, the
 * table written at the ids of the records that are not hidden -- (0 is the contract), <0 on error (no device, a null array, counts that do not add up, an
 * unknown kind).  outInfo: [0] whole items a wave holds under the mapping as built, [1] a workgroup, [2] live records, [3] workgroups launched.
 * giCDebugCompactRangesHost: the host form of the same kernel (gi_compact.h) against the same restatement, and with it the form the host compacts its own
 * arrays with, in place (compactRangesInPlaceHost; its table starts as the old one, which names every visible record at its old position); no device use. */
typedef struct GiCDebugCompactRange { uint32_t count, live, delta[3], hidden; } GiCDebugCompactRange;
int giCDebugCompactRanges(uint32_t kind, const void* records, uint32_t recordCount, const GiCDebugCompactRange* ranges, uint32_t rangeCount, uint32_t outInfo[4]);
int giCDebugCompactRangesHost(uint32_t kind, const void* records, uint32_t recordCount, const GiCDebugCompactRange* ranges, uint32_t rangeCount, uint32_t outInfo[4]);
/* [ext] [debug] what a built scene holds of the flat tree (GI_C_SCENE_OPTION_TLAS_ONLY): out[0] = 1 for the two-level layout, out[1] = 1 when the scene was built
 * without the flat tree, out[2] = flat nodes resident on device copy `device`, out[3] = bytes of flat nodes the host copy holds.  GI_C_OK, or GI_C_ERROR for a
 * scene that has not been built or a device copy that does not exist. */
int giCDebugSceneFlatTreeState(const GiCScene* scene, uint32_t device, uint64_t out[4]);
/* [ext] [debug] the flat triangle records, the id table (scene-order id -> flat record) and the per-instance traversal records resident on device
 * `deviceIndex` of a scene rendered at least once, downloaded and checked.  Returns the number of violations of: the ids of the records of visible instances
 * are a permutation of [0, visible triangles); the table names each of them at its id; its instance's triBase + prim is its id; records of hidden instances
 * have zero edges (0), <0 on error.  A mesh retired by a topology update in place counts as a hidden one: its ids are skipped; so does the storage
 * slot a retired instance left (GI_C_SCENE_OPTION_TLAS_INSTANCES) until a grow of its mesh takes it.  out[0]: visible triangles, [1] resident triangles, [2] hidden instances, [3] 1 when the two-level layout is in use (0:
 * nothing was compared). */
int giCDebugSceneFlatIdCheck(const GiCScene* scene, uint32_t deviceIndex, uint32_t* out /* 4 */);
/* [ext] [debug] device check of the kernels of a visibility update of the two-level layout (gi_patch.hip k_patch_visibility2 / k_patch_inst_trav).  The
 * caller describes `instanceCount` instances in scene order: faceCounts[i] triangles each, hiddenBefore[i] / hiddenAfter[i] != 0 where the instance is hidden
 * before / after the edit.  The hook makes synthetic flat records of all of them in a shuffled order drawn from `seed`, the state a build and the edits
 * before leave (ids over the instances visible before, zero edges and stale ids in the hidden ones, a table with stale words), applies the edit by both
 * kernels and by the host form of the same code (gi_vispatch.h), and checks the host form against the numbering a fresh build of the instances visible
 * after gives.  Returns the number of words of TriRec::origId, the table and InstTrav::triBase (and of the records' edges) that differ between device and
 * host form, plus the host form's violations of that numbering (0 is the contract), <0 on error.  outTris: resident triangles. */
int giCDebugPatchVisibilityTwoLevel(const uint32_t* faceCounts, const uint8_t* hiddenBefore, const uint8_t* hiddenAfter, uint32_t instanceCount, uint32_t seed,
                                    uint32_t* outTris);
/* [ext] what the last scene sync derived from the visible meshes' materials, the state that picks a render's kernel variants: out[0] the material classes in
 * use (one bit each), [1] those with a textured material, [2] and [3] the same per shade class, [4] 1 when some visible triangle has cutout opacity.  Host
 * only: no device work. */
int giCDebugSceneClassState(const GiCScene* scene, uint32_t* out /* 5 */);
/* [ext] the plain UsdPreviewSurface variant of the fused path kernel: out[0] what every UsdPreviewSurface material of the visible meshes has in common, as the
 * last scene sync derived it -- bit 0: clearcoat is the word of +0.0f in every one; 0 when one of them binds a texture or a primvar, or the scene has none --
 * and out[1] the traits the fused kernel of the scene's last render was
 * compiled for (0: the general kernel ran -- $GATLING_OPTIONS ups_plain=0, next-event estimation, other classes in use, a counting build --, or no fused
 * kernel).  Host only: no device work. */
int giCDebugSceneUpsPlain(const GiCScene* scene, uint32_t* out /* 2 */);
/* [ext] out[0] of giCDebugSceneUpsPlain for a scene whose visible meshes would use exactly the `count` materials of `descs`.  derive != 0: the descriptions are
 * what giCCreateMaterial takes; 0: `p` holds derived records word for word.  `flags` bit 31 marks a material with a bound input.  Host only: no scene. */
int giCDebugUpsTraits(const GiCMaterialDesc* descs, uint32_t count, int derive, uint32_t* out /* 1 */);
/* [ext] leaf lift (GI_C_SCENE_OPTION_LEAF_LIFT): out[0] the leaf slots the scene's last build moved into free slots of their parent's parent node (0: the
 * option or $GATLING_OPTIONS leaf_lift=0, a scene outside the pass -- beyond LDS, two-level, deeper than a root and one level, device-built --, or a tree the
 * model finds nothing to gain on), out[1] the levels of the flat tree (1: a root alone).  Host only: no device work. */
int giCDebugSceneLeafLift(const GiCScene* scene, uint32_t* out /* 2 */);
/* [ext] host-only: the pass itself.  treeNodes == NULL: the host builder's tree over `triCount` triangles (9 floats each: v0, v1, v2; ids = positions), then
 * the pass as `mode` says -- 0: not run, 1: run, -1: as a scene build would ($GATLING_OPTIONS leaf_lift, default on, and the LDS limits).  treeNodes != NULL:
 * `treeNodeCount` 80-byte nodes of a tree of `treeDepth` levels, breadth-first, over the triangles in THAT tree's leaf order (ids = positions), and the pass
 * run over it as `mode` says.  outNodes: room for `nodeCap` nodes (an error when the tree has more); outOrder: `triCount` ids, the leaf order of the result;
 * outInfo[0] nodes, [1] levels, [2] leaf slots moved, [3] triangles the tree references; outCost[0] / [1]: the model cost before / after the pass.
 * Returns the violations of the result's conservativeness contract as giCDebugValidateBvh counts them (0 = none), <0 on error. */
int giCDebugLeafLift(const float* triVerts, uint32_t triCount, int32_t mode, const void* treeNodes, uint32_t treeNodeCount, uint32_t treeDepth,
                     void* outNodes, uint32_t nodeCap, uint32_t* outOrder, uint32_t* outInfo /* 4 */, double* outCost /* 2 */);
/* [ext] cooked nodes ($GATLING_OPTIONS node_cook, default 1): out[0] is 1 when the fused kernel of the scene's last render ran a variant that stages its nodes
 * in cooked form -- each child's hit-mask word in a table, occupied slots first -- and 0 otherwise: node_cook=0, next-event estimation, a class mix, textures,
 * cutouts, a counting build, a tree whose cooked image would cost a resident block, or no fused kernel.  Host only: no device work. */
int giCDebugSceneNodeCook(const GiCScene* scene, uint32_t* out /* 1 */);
/* [ext] host-only: the cooked image of `nodeCount` 80-byte nodes as a block of the fused kernel stages it: nodeCount records of 112 bytes, then the octant area
 * of `octBlocks` blocks of 256 bytes (octBlocks < 0: what a tree of that many nodes can need, nodeCount - 1).  outImage: room for `imageCap` bytes, zeroed first
 * (blocks no node takes stay zero); outInfo[0] the bytes of the image, [1] the record stride, [2] the bytes of an octant block.  <0 on error. */
int giCDebugNodeCook(const void* nodes, uint32_t nodeCount, int32_t octBlocks, void* outImage, uint32_t imageCap, uint32_t* outInfo /* 3 */);
/* [ext] the cooked node test against the plain one on the device: pair i of `count` is ray i (8 floats: origin, direction, tMin, tBest) on node
 * i % nodeCount of `nodes` (1 .. 64 nodes of 80 bytes; they need not form a tree).  Returns the pairs whose hit groups differ in a bit, <0 on error. */
int64_t giCDebugCheckNodeCook(const void* nodes, uint32_t nodeCount, const float* rays, uint64_t count);
/* [ext] the fused path kernel's walk counters of the scene's last render, for renders with GI_C_SCENE_OPTION_COUNT_TRAVERSAL (all zero otherwise): out[0] trips
 * of all waves, [1 + k] the trips whose closest-hit loop reached step k (k = 7: every step from the eighth on), [9 + k] the lanes walking when those steps
 * began, [17] the steps that began with fewer than 8 lanes walking.  With $GATLING_OPTIONS walk_carry=K set explicitly a counting build carries walks as other
 * builds do, and these numbers are how a test sees it: [17] falls and [0] rises against K = 0, while the image and the per-ray counters stay put. */
int giCDebugPathWalkStats(const GiCScene* scene, uint64_t* out /* 18 */);
/* [ext] the fused path kernel's glossy-lobe counters of the scene's last render, for renders with GI_C_SCENE_OPTION_COUNT_TRAVERSAL (all zero otherwise): out[0]
 * hits shaded, [1] those that drew a glossy lobe of a UsdPreviewSurface material (coat or specular), [2] trips of all waves that shaded at least one such hit.
 * With $GATLING_OPTIONS lobe_park=N set explicitly a counting build parks such hits as other builds do, and the rest is how a test sees it: [3] LITE trips (glossy
 * hits set aside), [4] FULL trips (parked and own glossy hits shaded together), [5] hits parked, [6] records adopted, [7] trips whose shade ran again as FULL
 * on the spot because the lot could not take their glossy hits, [8] the hits shaded in those second passes.  [3] .. [8] are zero with lobe_park=0 or the key
 * absent; image and per-ray counters are the same whatever N. */
int giCDebugPathLobeStats(const GiCScene* scene, uint64_t* out /* 9 */);
/* [ext] the fused path kernel's triangle-ring counters of the scene's last render, for renders with GI_C_SCENE_OPTION_COUNT_TRAVERSAL (all zero otherwise):
 * out[0] triangle batches of the closest-hit loops, [1] the (ray, triangle) pairs tested in them, [2] the batches that held fewer than 64 pairs, [3] end-of-loop
 * flushes (a loop that ended with pairs pending), [4] steps whose pairs were appended by ballot rounds because the ring had no room for them at once.  With
 * $GATLING_OPTIONS ring_carry=1 set explicitly a counting build carries the ring across the steps of a trip as other builds do: partial batches then happen in
 * flushes only, at most one per trip.  With ring_carry=0 or the key absent every step ends with the ring empty and [3] is zero; the image is the same. */
int giCDebugPathRingStats(const GiCScene* scene, uint64_t* out /* 5 */);
/* [ext] how full the per-lane traversal stack got in the scene's last render, for renders with GI_C_SCENE_OPTION_COUNT_TRAVERSAL (all zero otherwise): out[0] the
 * most entries a closest-hit walk held -- the stack pointer after a push, maximum over every walk of the render --, [1] the same for the shadow walks, [2] the
 * stack rows of the traversal variant that ran (the fused path kernel and the LDS-resident trace kernel: 4 or 8; the persistent trace kernel: 8, 12 or 16),
 * [3] the entries that went to the scratch spill at most (trees deeper than 16 levels; else 0).  A walk pushes at most one entry per tree level below the
 * root, so [0] and [1] never exceed that depth.  Only [0] and [1] are counted on the device; [2] and [3] are DERIVED on the host from the rule the launch
 * dispatches by and from [0] / [1], not reported by the kernel that ran.  The primary device's walks only: on a scene spread over several devices the
 * other devices' shares are not in the maximum.  Counted by the fused path kernel and the two flat trace kernels; the two-level walk and the AOV kernel have no
 * such counter ([0] and [1] stay 0 for a two-level scene). */
int giCDebugTraversalStackHigh(const GiCScene* scene, uint32_t* out /* 4 */);
/* [ext] where the fused path kernel keeps parked hits for a BVH8 of `bvhDepth` levels below the root: out[0] traversal-stack rows per lane, [1] the first row
 * no walk reaches, [2] the records that fit in the rows from there on (0: parking is off for such a tree), [3] the dynamic LDS bytes of a launch for a scene of
 * nodeCount nodes and triCount triangles -- the rows and nothing else: parked hits add no LDS.  Host only: no device work, no scene. */
int giCDebugPathLot(uint32_t bvhDepth, uint32_t nodeCount, uint32_t triCount, uint32_t* out /* 4 */);
/* [ext] the miss rectangle of a whole-frame render: out = x0, y0, x1, y1, image columns [x0, x1) and rows [y0, y1) outside which every camera ray the settings'
 * sampling can produce for a pixel misses `bounds` (min xyz, max xyz) -- the fused path kernel gives such pixels no work.  The whole frame when no pixel can be
 * ruled out (depth of field with a lens radius, the camera inside or beside the bounds); 0, 0, 0, 0 when every pixel is (the camera looks away).  Host only: no
 * device work, no scene. */
int giCDebugMissRect(const float* bounds /* 6 */, const GiCCameraDesc* camera, const GiCRenderSettings* settings, uint32_t width, uint32_t height,
                     uint32_t* out /* 4 */);
/* [ext] [debug] the kernel of the sample-moments AOV (GI_C_AOV_EXT_MOMENTS; gi_moments.hip k_moments) over a synthetic per-sample buffer: a tile of
 * width x rows pixels (the whole image), `bufferSamples` Float32Vec4 records per pixel in `samples` -- [pixel][bufferSamples] with pixelMajor != 0, else
 * [bufferSamples][pixel] -- of which the samples [first, first + count) of every pixel are folded (first + count <= bufferSamples; a look-ahead window's slice
 * has first > 0).  prevM != NULL: width x rows records the fold continues from; NULL: from zero.  rect != NULL: x0, y0, x1, y1 -- a pixel outside columns
 * [x0, x1) and rows [y0, y1) has no records: each of its `count` samples is the constant missRgb (three finite values >= 0).  outM: width x rows records
 * (S1, S2, n, 0).  GI_C_OK, or GI_C_ERROR with a message (no device, a NULL or empty argument, a slice outside the buffer, more than 2^32 - 1 records, a
 * rectangle outside the image).  giCDebugSampleMomentsHost: the host form of the same per-pixel code (gi_moments.h); no device, works without giCInitialize. */
typedef struct GiCDebugMomentsDesc {
  uint32_t width, rows, bufferSamples, first, count, pixelMajor;
} GiCDebugMomentsDesc;
int giCDebugSampleMoments(const GiCDebugMomentsDesc* desc, const float* samples, const float* prevM, const uint32_t* rect /* 4 */, const float* missRgb /* 3 */,
                          float* outM);
int giCDebugSampleMomentsHost(const GiCDebugMomentsDesc* desc, const float* samples, const float* prevM, const uint32_t* rect /* 4 */,
                              const float* missRgb /* 3 */, float* outM);

#ifdef __cplusplus
}
#endif
#endif
