"""ctypes binding of the product library ``gatling_amd/libgatling_gi.so`` (C ABI: ``include/gi_c.h``).

This is the harness-side mirror of the reference's gi interface
(``/root/reference/src/gi/gtl/gi/Gi.h:199-261``): same entry points, same argument meaning.  There is no CPU
fallback -- if the HIP library is missing or no GPU is visible, loading / ``giCInitialize`` raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .scene import P_COUNT, SceneDesc, RenderSettings

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgatling_gi.so")
if os.environ.get("GATLING_GI_LIB"):  # experiments: a variant build of the same library (tools/build_variant.py), e.g. other kernel compile flags
    LIB_PATH = os.path.abspath(os.environ["GATLING_GI_LIB"])

GI_C_OK = 0
AOV_COLOR = 0
AOV_EXT_MOMENTS = 0x100  # GI_C_AOV_EXT_MOMENTS: a binding id outside the GiCAovId enum (include/gi_c.h)
FORMAT_INT32, FORMAT_FLOAT32, FORMAT_FLOAT32_VEC4 = 0, 1, 2
OPTION_COUNT_TRAVERSAL, OPTION_KERNEL_TIMERS, OPTION_POOL_SLOTS, OPTION_SAMPLE_BUFFER_MB, OPTION_TRACE_DYNAMIC, OPTION_TWO_LEVEL, OPTION_FUSED_PATH, OPTION_DEVICES = 1, 2, 3, 4, 5, 6, 7, 8
OPTION_SAMPLE_LOOKAHEAD = 10  # N >= 2: a progressive call may trace the samples of up to N calls in one batch (include/gi_c.h); 0 / 1 = off (default)
OPTION_VERTEX_UPDATES = 12  # 1: vertex edits (giCSetMeshVertices) of meshes of the built scene refit the resident BVH on the device instead of rebuilding the scene (include/gi_c.h); 0 = off (default)
OPTION_VISIBILITY_UPDATES = 11  # 1: visibility edits of meshes of the built scene are applied to the resident scene instead of rebuilding it (include/gi_c.h); 0 = off (default)
OPTION_TOPOLOGY_UPDATES = 13  # 1: meshes created and destroyed after the build are appended to / retired from the resident scene instead of rebuilding it (include/gi_c.h); 0 = off (default)
OPTION_RESYNC_REFITS = 14  # 1 (with options 12 and 13): a destroyed and a created mesh with the same faces become a vertex refit of the resident records instead of a retire + append (include/gi_c.h); 0 = off (default)
OPTION_INSTANCE_UPDATES = 15  # 1 (with option 13): new instance ids or another instance count of a built mesh are applied to the resident scene instead of rebuilding it (include/gi_c.h); 0 = off (default)
OPTION_TLAS_UPDATES = 16  # 1: transform edits of a built two-level scene (OPTION_TWO_LEVEL) are applied to the resident scene -- moved instances' records, a new TLAS, a refit of the flat tree -- instead of rebuilding it (include/gi_c.h); 0 = off (default)
OPTION_BLAS_UPDATES = 17  # 1: vertex edits of a built two-level scene are applied to the resident scene -- the mesh's BLAS refitted on the device, a new TLAS, a refit of the flat tree -- instead of rebuilding it; read only with OPTION_VERTEX_UPDATES wanted (include/gi_c.h); 0 = off (default)
OPTION_TLAS_VISIBILITY = 18  # 1: visibility edits of a built two-level scene are applied to the resident scene -- ids, the id table and the instances' id bases renumbered on the device, a new TLAS over the visible instances -- instead of rebuilding it; read only with OPTION_VISIBILITY_UPDATES wanted (include/gi_c.h); 0 = off (default)
OPTION_TLAS_ONLY = 19  # 1: a scene that takes the two-level layout (OPTION_TWO_LEVEL 1, or 2^26 flattened triangles) is built without the flat BVH8 -- the flat records stay in scene order, the non-colour AOVs walk the TLAS (k_aov2), the scene bounds come from the instance boxes and the edits in place of options 16 - 18 run without the flat refit; read at the scene build only (include/gi_c.h); 0 = off (default)
OPTION_TLAS_TOPOLOGY = 20  # 1: mesh creations and destructions on a built two-level scene without the flat tree (OPTION_TLAS_ONLY) are applied to the resident scene -- a destroyed mesh retired as a hidden one, a created mesh appended: one BLAS from the host, its shading records, BLAS triangles, flat records, face ids and id-table words made on the device (gi_append.hip) -- instead of rebuilding it; read only with OPTION_TOPOLOGY_UPDATES wanted (include/gi_c.h); 0 = off (default)
OPTION_TLAS_INSTANCES = 21  # 1: instance-id and instance-count edits of built meshes on a built two-level scene without the flat tree (OPTION_TLAS_ONLY) are applied to the resident scene -- retired instances hidden and their storage slots reused by later grows of the same mesh, new instances' flat records made on the device in one launch (gi_instances.hip) -- instead of rebuilding it; read only with OPTION_TOPOLOGY_UPDATES, OPTION_INSTANCE_UPDATES and OPTION_TLAS_TOPOLOGY wanted (include/gi_c.h); 0 = off (default)
OPTION_TLAS_DEVICE_BUILD = 22  # 1: the edits in place of a two-level scene (options 16 - 18, 20, 21) build their TLAS on the primary device (gi_tlas_build.hip: Morton sort, PLOC, depth-bounded cost-optimal collapse) instead of with the host builder, which remains the fallback; read only where such an edit is applied (include/gi_c.h); 0 = off (default)
OPTION_BVH_BUILD = 9  # 0 = host BVH builder (default), 1 = device builder (flat-layout scenes of more than 128 triangles)


class GiCCameraDesc(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("forward", C.c_float * 3), ("up", C.c_float * 3), ("vfov", C.c_float),
                ("fStop", C.c_float), ("focusDistance", C.c_float), ("focalLength", C.c_float), ("clipStart", C.c_float),
                ("clipEnd", C.c_float), ("exposure", C.c_float)]


class GiCMeshDesc(C.Structure):
    _fields_ = [("faceCount", C.c_uint32), ("faces", C.c_void_p), ("faceIds", C.c_void_p), ("id", C.c_int32),
                ("isDoubleSided", C.c_int32), ("isLeftHanded", C.c_int32), ("name", C.c_char_p), ("maxFaceId", C.c_uint32),
                ("vertexCount", C.c_uint32), ("vertices", C.c_void_p)]


class GiCRenderSettings(C.Structure):
    _fields_ = [("clippingPlanes", C.c_int32), ("depthOfField", C.c_int32), ("domeLightCameraVisible", C.c_int32),
                ("filterImportanceSampling", C.c_int32), ("frame", C.c_float), ("jitteredSampling", C.c_int32),
                ("lightIntensityMultiplier", C.c_float), ("maxBounces", C.c_uint32), ("maxSampleValue", C.c_float),
                ("maxVolumeWalkLength", C.c_uint32), ("mediumStackSize", C.c_uint32), ("metersPerSceneUnit", C.c_float),
                ("nextEventEstimation", C.c_int32), ("progressiveAccumulation", C.c_int32), ("rrBounceOffset", C.c_uint32),
                ("rrInvMinTermProb", C.c_float), ("spp", C.c_uint32), ("time", C.c_float)]


class GiCAovBinding(C.Structure):
    _fields_ = [("aovId", C.c_int32), ("clearValue", C.c_uint8 * 16), ("renderBuffer", C.c_void_p)]


class GiCRenderParams(C.Structure):
    _fields_ = [("aovBindings", C.POINTER(GiCAovBinding)), ("aovBindingCount", C.c_uint32), ("camera", GiCCameraDesc),
                ("domeLight", C.c_void_p), ("renderSettings", GiCRenderSettings), ("scene", C.c_void_p),
                ("rowBegin", C.c_uint32), ("rowEnd", C.c_uint32), ("rowStride", C.c_uint32)]


class GiCMaterialDesc(C.Structure):
    _fields_ = [("klass", C.c_uint32), ("flags", C.c_uint32), ("p", C.c_float * P_COUNT)]


class GiCRenderStats(C.Structure):
    _fields_ = [("renderMs", C.c_double), ("bvhBuildMs", C.c_double), ("uploadMs", C.c_double), ("traceMs", C.c_double),
                ("shadeMs", C.c_double), ("raygenMs", C.c_double), ("shadowMs", C.c_double),
                ("samples", C.c_uint64), ("segments", C.c_uint64), ("shadowRays", C.c_uint64), ("nodesVisited", C.c_uint64),
                ("trisTested", C.c_uint64), ("shadowNodesVisited", C.c_uint64), ("shadowTrisTested", C.c_uint64),
                ("iterations", C.c_uint32), ("traceLaunches", C.c_uint32), ("nodeCount", C.c_uint32), ("triangleCount", C.c_uint32),
                ("fusedPath", C.c_uint32), ("batches", C.c_uint32), ("poolSlots", C.c_uint32), ("inactiveTriangleCount", C.c_uint32)]


class GiCLookaheadStats(C.Structure):
    _fields_ = [("windowCalls", C.c_uint32), ("windowServed", C.c_uint32), ("traced", C.c_uint32), ("reserved", C.c_uint32),
                ("windowsTraced", C.c_uint64), ("callsServed", C.c_uint64), ("windowsDiscarded", C.c_uint64), ("samplesUnused", C.c_uint64)]


# giCDenoise (include/gi_c.h): where the inputs come from
DENOISE_SOURCE_AUTO, DENOISE_SOURCE_HOST, DENOISE_SOURCE_HOST_FORM = 0, 1, 2
# (GiCDenoiseStats.deviceInputs / sentInputs are bit masks: 1 colour, 2 normal, 4 depth, 8 albedo)


class GiCDenoiseParams(C.Structure):
    _fields_ = [("color", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("output", C.c_void_p),
                ("iterations", C.c_uint32), ("normalSquarings", C.c_uint32), ("sigmaColor", C.c_float), ("sigmaDepth", C.c_float),
                ("backgroundDepth", C.c_float), ("albedoFloor", C.c_float), ("source", C.c_int32)]


class GiCDenoiseVarianceParams(C.Structure):
    _fields_ = [("base", GiCDenoiseParams), ("moments", C.c_void_p), ("sigmaVariance", C.c_float), ("varianceFloor", C.c_float), ("minSamples", C.c_uint32)]


class GiCDenoiseStats(C.Structure):
    _fields_ = [("source", C.c_int32), ("deviceInputs", C.c_uint32), ("sentInputs", C.c_uint32), ("iterations", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("bytesSent", C.c_uint64), ("prepareMs", C.c_double), ("passMs", C.c_double * 6),
                ("copyMs", C.c_double), ("sendMs", C.c_double), ("totalMs", C.c_double)]


# every symbol include/gi_c.h declares: (name, restype, argtypes)
_P, _F, _U, _I = C.c_void_p, C.c_float, C.c_uint32, C.c_int32
_FP = C.POINTER(C.c_float)
class GiCTextureDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgba", C.c_void_p)]


class GiCTextureBinding(C.Structure):
    _fields_ = [("texture", C.c_void_p), ("wrapS", C.c_int32), ("wrapT", C.c_int32), ("channel", C.c_int32),
                ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


class GiCPrimvarData(C.Structure):
    _fields_ = [("name", C.c_char_p), ("type", C.c_int32), ("interpolation", C.c_int32), ("data", C.c_void_p), ("dataSize", C.c_uint64)]



# asset reader / image loader hooks (include/gi_c.h: giCRegisterAssetReader, giCSetImageLoader)
ASSET_OPEN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_char_p)
ASSET_SIZE = C.CFUNCTYPE(C.c_uint64, C.c_void_p, C.c_void_p)
ASSET_DATA = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_void_p)
ASSET_CLOSE = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)


class GiCAssetReader(C.Structure):
    _fields_ = [("user", C.c_void_p), ("open", ASSET_OPEN), ("size", ASSET_SIZE), ("data", ASSET_DATA), ("close", ASSET_CLOSE)]


class GiCDecodedImage(C.Structure):
    _fields_ = [("format", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("reserved", C.c_uint32), ("pixels", C.c_void_p), ("handle", C.c_void_p)]


IMAGE_LOAD = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(GiCDecodedImage))
IMAGE_RELEASE = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(GiCDecodedImage))
IMAGE_RGBA8_UNORM, IMAGE_RGB16_FLOAT, IMAGE_RGBA16_FLOAT, IMAGE_R32_FLOAT, IMAGE_RGBA32_FLOAT = 1, 2, 3, 4, 5


class GiCImageLoader(C.Structure):
    _fields_ = [("user", C.c_void_p), ("load", IMAGE_LOAD), ("release", IMAGE_RELEASE)]


SYMBOLS = [
    ("giCInitialize", C.c_int, [C.c_int]), ("giCInitializeDevices", C.c_int, [C.POINTER(C.c_int32), C.c_uint32]), ("giCGetDeviceCount", C.c_uint32, []), ("giCGetApiVersion", C.c_uint32, []), ("giCGetDevicePeerAccess", C.c_int32, [C.c_uint32]), ("giCTerminate", None, []), ("giCGetLastError", C.c_char_p, []),
    ("giCCreateMaterial", _P, [_P, C.c_char_p, C.POINTER(GiCMaterialDesc)]), ("giCDestroyMaterial", None, [_P]),
    ("giCCreateMesh", _P, [_P, C.POINTER(GiCMeshDesc)]), ("giCSetMeshTransform", None, [_P, _FP]),
    ("giCSetMeshInstanceTransforms", None, [_P, _U, _FP]), ("giCSetMeshInstanceIds", None, [_P, _U, C.POINTER(C.c_int32)]),
    ("giCSetMeshMaterial", None, [_P, _P]), ("giCSetMeshVisibility", None, [_P, _I]), ("giCSetMeshVertices", C.c_int, [_P, _U, _P]), ("giCDestroyMesh", None, [_P]),
    ("giCRender", C.c_int, [C.POINTER(GiCRenderParams)]),
    ("giCCreateScene", _P, []), ("giCDestroyScene", None, [_P]),
    ("giCCreateSphereLight", _P, [_P]), ("giCDestroySphereLight", None, [_P, _P]), ("giCSetSphereLightPosition", None, [_P, _FP]),
    ("giCSetSphereLightBaseEmission", None, [_P, _FP]), ("giCSetSphereLightRadius", None, [_P, _F, _F, _F]),
    ("giCSetSphereLightDiffuseSpecular", None, [_P, _F, _F]),
    ("giCCreateDistantLight", _P, [_P]), ("giCDestroyDistantLight", None, [_P, _P]), ("giCSetDistantLightDirection", None, [_P, _FP]),
    ("giCSetDistantLightBaseEmission", None, [_P, _FP]), ("giCSetDistantLightAngle", None, [_P, _F]),
    ("giCSetDistantLightDiffuseSpecular", None, [_P, _F, _F]),
    ("giCCreateRectLight", _P, [_P]), ("giCDestroyRectLight", None, [_P, _P]), ("giCSetRectLightOrigin", None, [_P, _FP]),
    ("giCSetRectLightTangents", None, [_P, _FP, _FP]), ("giCSetRectLightBaseEmission", None, [_P, _FP]),
    ("giCSetRectLightDimensions", None, [_P, _F, _F]), ("giCSetRectLightDiffuseSpecular", None, [_P, _F, _F]),
    ("giCCreateDiskLight", _P, [_P]), ("giCDestroyDiskLight", None, [_P, _P]), ("giCSetDiskLightOrigin", None, [_P, _FP]),
    ("giCSetDiskLightTangents", None, [_P, _FP, _FP]), ("giCSetDiskLightBaseEmission", None, [_P, _FP]),
    ("giCSetDiskLightRadius", None, [_P, _F, _F]), ("giCSetDiskLightDiffuseSpecular", None, [_P, _F, _F]),
    ("giCCreateDomeLight", _P, [_P, C.c_char_p]), ("giCDestroyDomeLight", None, [_P]), ("giCSetDomeLightRotation", None, [_P, _FP]),
    ("giCSetDomeLightBaseEmission", None, [_P, _FP]), ("giCSetDomeLightDiffuseSpecular", None, [_P, _F, _F]),
    ("giCSetDomeLightTexture", None, [_P, _P]),
    ("giCCreateTexture", _P, [_P, C.POINTER(GiCTextureDesc)]), ("giCDestroyTexture", None, [_P]),
    ("giCCreateTextureFromFile", _P, [_P, C.c_char_p, _I]),
    ("giCDebugDecodeImage", C.c_int, [C.c_char_p, _I, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _FP, C.c_uint64]),
    ("giCRegisterAssetReader", None, [C.POINTER(GiCAssetReader)]), ("giCSetImageLoader", None, [C.POINTER(GiCImageLoader)]),
    ("giCSetMaterialTexture", C.c_int, [_P, _I, C.POINTER(GiCTextureBinding)]),
    ("giCSetMaterialTextureTransform", C.c_int, [_P, _I, _FP]),
    ("giCSetMeshPrimvars", C.c_int, [_P, _U, C.POINTER(GiCPrimvarData)]), ("giCSetMeshInstancerPrimvars", C.c_int, [_P, _U, C.POINTER(GiCPrimvarData)]),
    ("giCSetMaterialPrimvarInput", C.c_int, [_P, _I, C.c_char_p]),
    ("giCCreateRenderBuffer", _P, [_U, _U, _I]), ("giCDestroyRenderBuffer", None, [_P]), ("giCGetRenderBufferMem", _P, [_P]),
    ("giCGetRenderBufferDeviceMem", _P, [_P]), ("giCSetRenderBufferDeviceOnly", None, [_P, _I]),
    ("giCCreateHostRenderBuffer", _P, [_U, _U, _I]),
    ("giCDenoiseVarianceDefaults", None, [C.POINTER(GiCDenoiseVarianceParams)]), ("giCDenoiseVariance", C.c_int, [C.POINTER(GiCDenoiseVarianceParams)]),
    ("giCDenoiseDefaults", None, [C.POINTER(GiCDenoiseParams)]), ("giCDenoise", C.c_int, [C.POINTER(GiCDenoiseParams)]),
    ("giCGetDenoiseStats", C.c_int, [C.POINTER(GiCDenoiseStats)]),
    ("giCGetRenderStats", C.c_int, [_P, C.POINTER(GiCRenderStats)]), ("giCSetSceneOption", C.c_int, [_P, _I, _I]),
    ("giCGetLookaheadStats", C.c_int, [_P, C.POINTER(GiCLookaheadStats)]),
    ("giCTraceRays", C.c_int, [_P, _U, _FP, _FP, _F, _F, _FP, C.POINTER(C.c_int32)]),
    ("giCDebugEvalBsdf", C.c_int, [C.POINTER(GiCMaterialDesc), _U, _FP, _FP]),
    ("giCDebugShadeClass", C.c_int, [C.POINTER(GiCMaterialDesc)]),
    ("giCDebugCheckSqrt", C.c_int64, [C.c_uint32, C.c_uint64]),
    ("giCDebugCheckDiv", C.c_int64, [C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("giCDebugValidateBvh", C.c_int, [_FP, _U, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("giCDebugValidatePartitionedBvh", C.c_int, [_FP, _U, _U, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("giCDebugValidateSceneBvh", C.c_int, [_P, _U, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    ("giCDebugTexRuntime", C.c_int, [_FP, _U, _U, _U, _U, _FP, _FP]),
    ("giCDebugEditDirtyFlags", C.c_int32, [_I, _I]), ("giCDebugSceneUpdateCounts", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("giCDebugSceneVisibilityUpdateCount", C.c_int, [_P, C.POINTER(C.c_uint64)]), ("giCDebugSceneClassState", C.c_int, [_P, C.POINTER(C.c_uint32)]),
    ("giCDebugSceneUpsPlain", C.c_int, [_P, C.POINTER(C.c_uint32)]), ("giCDebugUpsTraits", C.c_int, [C.POINTER(GiCMaterialDesc), _U, C.c_int, C.POINTER(C.c_uint32)]),
    ("giCDebugSceneLeafLift", C.c_int, [_P, C.POINTER(C.c_uint32)]),
    ("giCDebugSceneNodeCook", C.c_int, [_P, C.POINTER(C.c_uint32)]),
    ("giCDebugNodeCook", C.c_int, [_P, _U, C.c_int32, _P, _U, C.POINTER(C.c_uint32)]),
    ("giCDebugCheckNodeCook", C.c_int64, [_P, _U, _FP, C.c_uint64]),
    ("giCDebugLeafLift", C.c_int, [_FP, _U, C.c_int32, _P, _U, _U, _P, _U, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_double)]),
    ("giCDebugSceneVertexUpdateCount", C.c_int, [_P, C.POINTER(C.c_uint64)]), ("giCDebugRefitBvh", C.c_int, [_FP, _FP, _U, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("giCDebugSceneRefitCheck", C.c_int, [_P, _U, C.POINTER(C.c_uint32)]),
    ("giCDebugSceneTopologyUpdateCount", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("giCDebugSceneResyncCount", C.c_int, [_P, C.POINTER(C.c_uint64)]), ("giCDebugGatherShade", C.c_int, [_P, _U, _P, _U]),
    ("giCDebugSceneShadeCheck", C.c_int, [_P, _U, C.POINTER(C.c_uint32)]),
    ("giCDebugSceneInstanceUpdateCount", C.c_int, [_P, C.POINTER(C.c_uint64)]), ("giCDebugCloneInstance", C.c_int, [_P, _U, _P, _U, _I, _FP, _FP]),
    ("giCDebugSceneTlasUpdateCount", C.c_int, [_P, C.POINTER(C.c_uint64)]), ("giCDebugSceneTlasCheck", C.c_int, [_P, _U, C.POINTER(C.c_uint32)]),
    ("giCDebugInstanceBounds", C.c_int, [_P, _U, _P, _U, _FP, _U, _FP, C.POINTER(C.c_uint32)]),
    ("giCDebugSceneBlasUpdateCount", C.c_int, [_P, C.POINTER(C.c_uint64)]), ("giCDebugSceneBlasCheck", C.c_int, [_P, _U, C.POINTER(C.c_uint32)]),
    ("giCDebugBlasRefit", C.c_int, [_P, _P, _U, _P, _U, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("giCDebugBlasRefitHost", C.c_int, [_P, _P, _U, _P, _U, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("giCDebugSceneTlasVisibilityUpdateCount", C.c_int, [_P, C.POINTER(C.c_uint64)]), ("giCDebugSceneFlatIdCheck", C.c_int, [_P, _U, C.POINTER(C.c_uint32)]),
    ("giCDebugSceneFlatTreeState", C.c_int, [_P, _U, C.POINTER(C.c_uint64)]),
    ("giCDebugSceneTlasTopologyUpdateCount", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("giCDebugAppendRecords", C.c_int, [_P, _U, _P, _U, _P, _U, _U, _FP, _U, _U, _U, _U, _U]),
    ("giCDebugAppendRecordsHost", C.c_int, [_P, _U, _P, _U, _P, _U, _U, _FP, _U, _U, _U, _U, _U]),
    ("giCDebugInstanceRecords", C.c_int, [_P, _U, _P, _U]),
    ("giCDebugInstanceRecordsHost", C.c_int, [_P, _U, _P, _U]),
    ("giCDebugSceneTlasInstanceUpdateStats", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("giCDebugSceneCompactionCount", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("giCDebugCompactRanges", C.c_int, [_U, _P, _U, _P, _U, C.POINTER(C.c_uint32)]),
    ("giCDebugCompactRangesHost", C.c_int, [_U, _P, _U, _P, _U, C.POINTER(C.c_uint32)]),
    ("giCDebugBuildTlasHost", C.c_int, [_FP, _U, _U, _U, C.POINTER(C.c_double)]),
    ("giCDebugBuildTlas", C.c_int, [_FP, _U, _U, _U, C.POINTER(C.c_double)]),
    ("giCDebugBuildBlasHost", C.c_int, [_P, _U, _P, _U, _U, _U, C.POINTER(C.c_double)]),
    ("giCDebugBuildBlas", C.c_int, [_P, _U, _P, _U, _U, _U, C.POINTER(C.c_double)]),
    ("giCDebugSceneBlasBuildStats", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("giCDebugSceneTlasBuildStats", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("giCDebugPatchVisibilityTwoLevel", C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _U, _U, C.POINTER(C.c_uint32)]),
    ("giCDebugPathWalkStats", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("giCDebugPathLobeStats", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("giCDebugPathRingStats", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("giCDebugPathLot", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("giCDebugTraversalStackHigh", C.c_int, [_P, C.POINTER(C.c_uint32)]),
    ("giCDebugBvhStackReach", C.c_int, [_FP, _U, _FP, _FP, _U, C.POINTER(C.c_uint32)]),
    ("giCDebugSampleMoments", C.c_int, [_P, _FP, _FP, C.POINTER(C.c_uint32), _FP, _FP]),
    ("giCDebugSampleMomentsHost", C.c_int, [_P, _FP, _FP, C.POINTER(C.c_uint32), _FP, _FP]),
    ("giCDebugMissRect", C.c_int, [_FP, C.POINTER(GiCCameraDesc), C.POINTER(GiCRenderSettings), _U, _U, C.POINTER(C.c_uint32)]),
]

_lib = None


def load_library():
    """Loads libgatling_gi.so and types every entry point.  Raises if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _fp(values):
    arr = (C.c_float * len(values))(*[float(v) for v in values])
    return arr


class GiError(RuntimeError):
    pass


def denoise_params(**params) -> GiCDenoiseParams:
    """giCDenoiseDefaults with the named fields replaced: iterations, normalSquarings, sigmaColor, sigmaDepth, backgroundDepth, albedoFloor, source."""
    p = GiCDenoiseParams()
    load_library().giCDenoiseDefaults(C.byref(p))
    for k, v in params.items():
        if k not in ("iterations", "normalSquarings", "sigmaColor", "sigmaDepth", "backgroundDepth", "albedoFloor", "source"):
            raise TypeError(f"denoise: unknown parameter {k!r}")
        setattr(p, k, v)
    return p


def denoise_stats() -> dict:
    """giCGetDenoiseStats: the last giCDenoise of the process -- the source it used, which inputs were read from their device copies and which were sent,
    the bytes sent, and the times of the prepare launch, every pass and the copy back (device events; the host form: host clock)."""
    s = GiCDenoiseStats()
    if load_library().giCGetDenoiseStats(C.byref(s)) != GI_C_OK:
        raise GiError("giCGetDenoiseStats failed")
    out = {name: getattr(s, name) for name, _ in GiCDenoiseStats._fields_ if name != "passMs"}
    out["passMs"] = [float(v) for v in s.passMs][:s.iterations]
    return out


VARIANCE_PARAMS = ("sigmaVariance", "varianceFloor", "minSamples")


def denoise_variance_params(**params) -> GiCDenoiseVarianceParams:
    """giCDenoiseVarianceDefaults with the named fields replaced: giCDenoiseParams' fields (into ``base``) and sigmaVariance, varianceFloor, minSamples."""
    p = GiCDenoiseVarianceParams()
    load_library().giCDenoiseVarianceDefaults(C.byref(p))
    p.base = denoise_params(**{k: v for k, v in params.items() if k not in VARIANCE_PARAMS})
    for k in VARIANCE_PARAMS:
        if k in params:
            setattr(p, k, params[k])
    return p


def denoise_variance(color, normal, depth, moments, albedo=None, host_form=False, **params):
    """giCDenoiseVariance over arrays: as ``denoise`` with ``moments`` float32 [h, w, 4] = (S1, S2, n, 0) (the "moments" AOV); the keyword parameters are
    giCDenoiseParams' fields and sigmaVariance, varianceFloor, minSamples."""
    return denoise(color, normal, depth, albedo, host_form, _moments=moments, **params)


def denoise(color, normal, depth, albedo=None, host_form=False, _moments=None, **params):
    """giCDenoise over arrays: color / normal / albedo float32 [h, w, 4], depth float32 [h, w]; returns the filtered image [h, w, 4].  ``host_form=True``
    runs the host form over host render buffers (no device, no giCInitialize); otherwise the arrays are sent to the device
    (GI_C_DENOISE_SOURCE_HOST: the library must be initialised) and the kernels of gi_denoise.hip run.  The keyword parameters are giCDenoiseParams' fields."""
    L = load_library()
    color = np.ascontiguousarray(color, np.float32)
    h, w = color.shape[:2]
    arrays = {"color": color, "normal": np.ascontiguousarray(normal, np.float32), "depth": np.ascontiguousarray(depth, np.float32)}
    if albedo is not None:
        arrays["albedo"] = np.ascontiguousarray(albedo, np.float32)
    if _moments is not None:
        arrays["moments"] = np.ascontiguousarray(_moments, np.float32)
    create = L.giCCreateHostRenderBuffer if host_form else L.giCCreateRenderBuffer
    bufs = {}
    try:
        for name, a in list(arrays.items()) + [("output", None)]:
            fmt = FORMAT_FLOAT32 if name == "depth" else FORMAT_FLOAT32_VEC4
            if a is not None and a.shape != ((h, w) if name == "depth" else (h, w, 4)):
                raise ValueError(f"denoise: {name} has shape {a.shape}")
            rb = create(w, h, fmt)
            if not rb:
                raise GiError("render buffer creation failed: " + L.giCGetLastError().decode())
            bufs[name] = rb
            if a is not None and a.nbytes:
                C.memmove(L.giCGetRenderBufferMem(rb), a.ctypes.data, a.nbytes)
        source = DENOISE_SOURCE_HOST_FORM if host_form else DENOISE_SOURCE_HOST
        vp = denoise_variance_params(source=source, **params) if _moments is not None else None
        p = vp.base if vp is not None else denoise_params(source=source, **params)
        p.color, p.normal, p.depth, p.albedo, p.output = bufs["color"], bufs["normal"], bufs["depth"], bufs.get("albedo"), bufs["output"]
        if vp is not None:
            vp.moments = bufs["moments"]
            if L.giCDenoiseVariance(C.byref(vp)) != GI_C_OK:
                raise GiError("giCDenoiseVariance failed: " + L.giCGetLastError().decode())
        elif L.giCDenoise(C.byref(p)) != GI_C_OK:
            raise GiError("giCDenoise failed: " + L.giCGetLastError().decode())
        out = np.empty((h, w, 4), np.float32)
        if out.nbytes:
            C.memmove(out.ctypes.data, L.giCGetRenderBufferMem(bufs["output"]), out.nbytes)
        return out
    finally:
        for rb in bufs.values():
            L.giCDestroyRenderBuffer(rb)


def debug_sample_moments(samples, pixel_major, width, rows, first=0, count=None, prev=None, rect=None, miss_rgb=None, host_only=False):
    """giCDebugSampleMoments: the kernel of the moments AOV (k_moments) over a synthetic per-sample buffer.  ``samples``: float32 [pixels, S, 4] with
    ``pixel_major`` else [S, pixels, 4], pixels = width * rows; the samples [first, first + count) of every pixel are folded (count defaults to the rest),
    from ``prev`` ([pixels, 4]) or from zero.  ``rect`` = (x0, y0, x1, y1): pixels outside it have no records, each sample of theirs is ``miss_rgb``.
    Returns M float32 [pixels, 4] = (S1, S2, n, 0).  host_only: giCDebugSampleMomentsHost, the host form of the same per-pixel code (no device)."""
    L = load_library()
    samples = np.ascontiguousarray(samples, np.float32)
    pixels = int(width) * int(rows)
    S = samples.shape[1] if pixel_major else samples.shape[0]
    assert samples.shape == ((pixels, S, 4) if pixel_major else (S, pixels, 4)), samples.shape
    d = (C.c_uint32 * 6)(int(width), int(rows), S, int(first), int(S - first if count is None else count), int(bool(pixel_major)))
    ptr = lambda a: None if a is None else a.ctypes.data_as(_FP)
    prev_a = None if prev is None else np.ascontiguousarray(prev, np.float32).reshape(pixels, 4)
    rect_a = None if rect is None else (C.c_uint32 * 4)(*[int(v) for v in rect])
    miss_a = None if miss_rgb is None else np.ascontiguousarray(miss_rgb, np.float32)
    out = np.empty((pixels, 4), np.float32)
    fn = L.giCDebugSampleMomentsHost if host_only else L.giCDebugSampleMoments
    if fn(d, ptr(samples), ptr(prev_a), rect_a, ptr(miss_a), ptr(out)) != GI_C_OK:
        raise GiError("giCDebugSampleMoments failed: " + L.giCGetLastError().decode())
    return out


def miss_rect(bounds, camera, rs: "RenderSettings", width: int, height: int):
    """giCDebugMissRect: (x0, y0, x1, y1) -- the image rectangle outside which every camera ray of a pixel misses `bounds` (min xyz, max xyz); the whole
    frame when nothing can be ruled out, (0, 0, 0, 0) when everything is.  Host only: needs neither a device nor giCInitialize."""
    L = load_library()
    out = (C.c_uint32 * 4)()
    cam, st = _camera(camera), _settings(rs)
    if L.giCDebugMissRect(_fp(bounds), C.byref(cam), C.byref(st), int(width), int(height), out) != GI_C_OK:
        raise GiError("giCDebugMissRect failed: " + L.giCGetLastError().decode())
    return tuple(int(v) for v in out)


def leaf_lift(tri_verts, mode: int = 1, tree_nodes=None, tree_depth: int = 0) -> dict:
    """giCDebugLeafLift: the leaf lift of small flat trees (leaf_lift.cpp) on the host.  Without `tree_nodes`: the host builder's BVH8 over `tri_verts` (n x 3 x 3
    triangles in scene order), then the pass as `mode` says -- 0: not run, 1: run, -1: as a scene build would (GATLING_OPTIONS leaf_lift, the LDS limits).  With
    `tree_nodes` (bytes or a uint8 array of 80-byte nodes, breadth-first, `tree_depth` levels): that tree over the triangles in ITS leaf order.  Returns
    {"violations", "nodes" (uint8, n x 80), "order" (ids in leaf order), "depth", "lifted", "active", "cost_before", "cost_after"}.  Host only."""
    import numpy as np
    L = load_library()
    v = np.ascontiguousarray(tri_verts, np.float32).reshape(-1, 9)
    given = None if tree_nodes is None else np.ascontiguousarray(np.frombuffer(bytes(tree_nodes), np.uint8)).reshape(-1, 80)
    cap = max(len(v), 1) + 1 if given is None else len(given)
    nodes = np.zeros((cap, 80), np.uint8); order = np.zeros(max(len(v), 1), np.uint32); info = np.zeros(4, np.uint32); cost = np.zeros(2, np.float64)
    rc = L.giCDebugLeafLift(v.ctypes.data_as(_FP), len(v), mode, None if given is None else given.ctypes.data_as(_P), 0 if given is None else len(given), tree_depth,
                            nodes.ctypes.data_as(_P), cap, order.ctypes.data_as(C.POINTER(C.c_uint32)), info.ctypes.data_as(C.POINTER(C.c_uint32)),
                            cost.ctypes.data_as(C.POINTER(C.c_double)))
    if rc < 0:
        raise GiError(f"giCDebugLeafLift failed ({rc})")
    return {"violations": rc, "nodes": nodes[:int(info[0])].copy(), "order": order[:len(v)].copy(), "depth": int(info[1]), "lifted": int(info[2]),
            "active": int(info[3]), "cost_before": float(cost[0]), "cost_after": float(cost[1])}


def node_cook(nodes, oct_blocks: int = -1) -> dict:
    """giCDebugNodeCook: the cooked image of `nodes` (bytes or a uint8 array of 80-byte nodes) as a block of the fused kernel stages it.  Returns {"records"
    (uint32, n x 28), "oct" (uint32, blocks x 8 octants x 8 children), "stride", "oct_block_bytes"}; `oct_blocks` < 0: the blocks a tree of n nodes can need,
    n - 1.  Host only."""
    import numpy as np
    L = load_library()
    given = np.ascontiguousarray(np.frombuffer(bytes(nodes), np.uint8)).reshape(-1, 80)
    n = len(given)
    blocks = max(n - 1, 0) if oct_blocks < 0 else int(oct_blocks)
    image = np.zeros(n * 28 + blocks * 64, np.uint32); info = np.zeros(3, np.uint32)
    if L.giCDebugNodeCook(given.ctypes.data_as(_P), n, int(oct_blocks), image.ctypes.data_as(_P), image.nbytes, info.ctypes.data_as(C.POINTER(C.c_uint32))) != GI_C_OK:
        raise GiError("giCDebugNodeCook failed: " + L.giCGetLastError().decode())
    assert int(info[0]) == image.nbytes and int(info[1]) == 112 and int(info[2]) == 256
    return {"records": image[:n * 28].reshape(n, 28).copy(), "oct": image[n * 28:].reshape(blocks, 8, 8).copy(), "stride": int(info[1]),
            "oct_block_bytes": int(info[2])}


def check_node_cook(nodes, rays) -> int:
    """giCDebugCheckNodeCook: on the device, the cooked node test against the plain one for the pairs (node i % n, ray i); `nodes`: 1 .. 64 nodes of 80 bytes,
    `rays`: m x 8 floats (origin, direction, tMin, tBest).  Returns the pairs whose hit groups differ in a bit."""
    import numpy as np
    L = load_library()
    given = np.ascontiguousarray(np.frombuffer(bytes(nodes), np.uint8)).reshape(-1, 80)
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    bad = L.giCDebugCheckNodeCook(given.ctypes.data_as(_P), len(given), r.ctypes.data_as(_FP), len(r))
    if bad < 0:
        raise GiError("giCDebugCheckNodeCook failed: " + L.giCGetLastError().decode())
    return int(bad)


def bvh_stack_reach(tri_verts, origins, dirs):
    """giCDebugBvhStackReach: (levels, nodes, reach) of the host builder's BVH8 over `tri_verts` (n x 3 x 3 world-space triangles in scene order) -- reach[i] is
    the most stack entries the traversal kernels' ordered walk holds for ray i.  The walk tests boxes only and culls nothing, so reach is an UPPER BOUND on
    what a device walk of the ray holds (exact for a ray that hits no triangle): it is for designing scenes and for pinning them against builder changes; that
    a render did fill a stack is shown by the device counter (Scene.traversal_stack_high).  Host only: needs neither a device nor giCInitialize."""
    import numpy as np
    L = load_library()
    v = np.ascontiguousarray(tri_verts, np.float32).reshape(-1, 9)
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    assert o.shape == d.shape
    out = np.zeros(2 + len(o), np.uint32)
    if L.giCDebugBvhStackReach(v.ctypes.data_as(_FP), len(v), o.ctypes.data_as(_FP), d.ctypes.data_as(_FP), len(o), out.ctypes.data_as(C.POINTER(C.c_uint32))) != 0:
        raise GiError("giCDebugBvhStackReach failed")
    return int(out[0]), int(out[1]), out[2:].copy()


def debug_gather_shade(vertices, faces) -> int:
    """giCDebugGatherShade: the shading records a vertex update gathers from the packed vertex records against the ones the scene build packs, for the mesh
    (`vertices`: VERTEX_DTYPE, `faces`: n x 3 indices).  Returns the number of differing records (0 is the contract).  Host only."""
    from .scene import VERTEX_DTYPE
    L = load_library()
    v = np.ascontiguousarray(vertices, VERTEX_DTYPE)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    n = L.giCDebugGatherShade(v.ctypes.data, len(v), f.ctypes.data, len(f))
    if n < 0:
        raise GiError("giCDebugGatherShade refused the mesh")
    return int(n)


def debug_clone_instance(vertices, faces, xform_a, xform_b, left_handed=False) -> int:
    """giCDebugCloneInstance: the records of the mesh (`vertices`: VERTEX_DTYPE, `faces`: n x 3 indices) flattened under the instance transform `xform_a` and
    cloned to `xform_b` (4 x 4, USD row vectors) by the function the device's clone kernel runs, against the scene build's records for `xform_b`.  Returns the
    number of differing records (0 is the contract).  Host only."""
    from .scene import VERTEX_DTYPE
    L = load_library()
    v = np.ascontiguousarray(vertices, VERTEX_DTYPE)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    a, b = (np.ascontiguousarray(x, np.float32).reshape(16) for x in (xform_a, xform_b))
    n = L.giCDebugCloneInstance(v.ctypes.data, len(v), f.ctypes.data, len(f), int(bool(left_handed)), a.ctypes.data_as(_FP), b.ctypes.data_as(_FP))
    if n < 0:
        raise GiError("giCDebugCloneInstance refused the mesh or a transform")
    return int(n)


OPTION_BLAS_DEVICE_BUILD = 23  # 1: the BLAS of a mesh of blas_device_min .. blas_device_max faces of a two-level scene is built on the primary device (gi_blas_build.hip: face boxes from the uploaded points, then the device TLAS builder's stages under a deeper budget) instead of with the host builder, which remains the fallback; read at the scene build and where option 20 applies a mesh create (include/gi_c.h); 0 = off (default)
OPTION_TLAS_COMPACTION = 24  # 1: before a topology or instancer edit in place of a two-level scene without the flat tree declines because retired triangles outnumber live ones (retired x 100 > live x GATLING_OPTIONS=tlas_compact_percent, default 100), the ranges earlier edits retired are compacted on the device (gi_compact.hip: one launch per array kind into new allocations, indices rebased, the TLAS rebuilt) and the edit goes on; read only where option 20 or 21 applies an edit (include/gi_c.h); 0 = off (default)
OPTION_LEAF_LIFT = 25  # -1 / 1: the flat tree of a scene the fused kernel walks out of LDS (LDS-resident, not two-level, a root and one level below it) goes through the leaf lift (leaf_lift.cpp) at the scene build; 0: the builder's tree, byte for byte (include/gi_c.h); default on; GATLING_OPTIONS=leaf_lift overrides it
TLAS_BUILD_TOO_DEEP = -2  # GI_C_TLAS_BUILD_TOO_DEEP


def debug_build_tlas(boxes, depth_budget=7, radius=16, host_only=False) -> dict:
    """giCDebugBuildTlasHost (`host_only`: no device is used) / giCDebugBuildTlas: the TLAS builder of edits in place (OPTION_TLAS_DEVICE_BUILD) over `boxes`
    (n x 6: min xyz, max xyz) with at most `depth_budget` levels and PLOC radius `radius`.  Returns {"violations": broken rules of the tree -- plus, for the
    device builder, node and item records that differ bytewise from the host form's -- (0 is the contract), or TLAS_BUILD_TOO_DEEP; "nodes", "depth",
    "passes", "cost" and "host_cost" (the SAH model cost of this tree and of the host builder's over the same boxes, by one function), "host_waits",
    "host_depth", "active"}."""
    L = load_library()
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    out = (C.c_double * 8)()
    fn = L.giCDebugBuildTlasHost if host_only else L.giCDebugBuildTlas
    v = fn(b.ctypes.data_as(_FP), len(b), int(depth_budget), int(radius), out)
    if v < 0 and v != TLAS_BUILD_TOO_DEEP:
        raise GiError("giCDebugBuildTlas failed: " + L.giCGetLastError().decode())
    return {"violations": int(v), "nodes": int(out[0]), "depth": int(out[1]), "passes": int(out[2]), "cost": float(out[3]), "host_cost": float(out[4]),
            "host_waits": int(out[5]), "host_depth": int(out[6]), "active": int(out[7])}


def debug_build_blas(vertices, faces, depth_budget=12, radius=16, host_only=False) -> dict:
    """giCDebugBuildBlasHost (`host_only`: no device is used) / giCDebugBuildBlas: the BLAS builder of OPTION_BLAS_DEVICE_BUILD over one mesh (`vertices`:
    VERTEX_DTYPE, `faces`: n x 3 indices) with at most `depth_budget` levels and PLOC radius `radius`.  Returns {"violations": broken rules of the tree -- plus,
    for the device builder, the node / order / mlo / mhi bytes that differ from the host form's -- (0 is the contract), or TLAS_BUILD_TOO_DEEP; "nodes",
    "depth", "passes", "cost" and "host_cost" (the SAH model cost of this tree and of the host builder's), "host_waits", "host_depth", "active",
    "conservative" (blasConservativeViolations), "rules" (depth within the budget, every usable face named once, unusable faces behind in input order,
    children behind parents), "levels" (level table), "bounds_bytes" (mlo / mhi against the host builder's), "tlas_records" (records that differ from the TLAS
    builder's host form over the same boxes; compared for depth_budget <= 7), "refit_bytes" (node bytes a refit over the unchanged points changes), "budget",
    "differing_bytes" (device against host form)}."""
    from .scene import VERTEX_DTYPE
    L = load_library()
    v = np.ascontiguousarray(vertices, VERTEX_DTYPE)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    out = (C.c_double * 16)()
    fn = L.giCDebugBuildBlasHost if host_only else L.giCDebugBuildBlas
    r = fn(v.ctypes.data, len(v), f.ctypes.data, len(f), int(depth_budget), int(radius), out)
    if r < 0 and r != TLAS_BUILD_TOO_DEEP:
        raise GiError("giCDebugBuildBlas failed: " + L.giCGetLastError().decode())
    return {"violations": int(r), "nodes": int(out[0]), "depth": int(out[1]), "passes": int(out[2]), "cost": float(out[3]), "host_cost": float(out[4]),
            "host_waits": int(out[5]), "host_depth": int(out[6]), "active": int(out[7]), "conservative": int(out[8]), "rules": int(out[9]), "levels": int(out[10]),
            "bounds_bytes": int(out[11]), "tlas_records": int(out[12]), "refit_bytes": int(out[13]), "budget": int(out[14]), "differing_bytes": int(out[15])}


def debug_instance_bounds(vertices, faces, xforms):
    """giCDebugInstanceBounds: the device kernels that make the world boxes of moved instances of a two-level scene (k_inst_bounds / k_inst_finish) over the
    mesh (`vertices`: VERTEX_DTYPE, `faces`: n x 3 indices) under each of `xforms` (k x 4 x 4, USD row vectors), against the host form of the same arithmetic.
    Returns (differing, boxes, status): the number of (box, status) pairs that differ bytewise (0 is the contract), the device's padded boxes (k x 6: min xyz,
    max xyz) and status words (k; 0 = usable).  Needs an initialised device."""
    from .scene import VERTEX_DTYPE
    L = load_library()
    v = np.ascontiguousarray(vertices, VERTEX_DTYPE)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    x = np.ascontiguousarray(xforms, np.float32).reshape(-1, 16)
    boxes = np.zeros((len(x), 6), np.float32)
    status = np.zeros(len(x), np.uint32)
    n = L.giCDebugInstanceBounds(v.ctypes.data, len(v), f.ctypes.data, len(f), x.ctypes.data_as(_FP), len(x), boxes.ctypes.data_as(_FP),
                                 status.ctypes.data_as(C.POINTER(C.c_uint32)))
    if n < 0:
        raise GiError("giCDebugInstanceBounds failed: " + L.giCGetLastError().decode())
    return int(n), boxes, status


def debug_blas_refit(vertices_a, vertices_b, faces, host_only=False):
    """giCDebugBlasRefit: one BLAS of the two-level layout is built over the mesh with points `vertices_a` (VERTEX_DTYPE; `faces`: n x 3 indices) and brought
    to `vertices_b` by the device kernels (k_blas_tris / k_blas_refit_level) and by the host form of the same arithmetic.  Returns (differing, nodes,
    violations): the node and record bytes that differ between device and host -- with the same positions in both, plus those that differ from the build's
    -- (0 is the contract), the BLAS's node count, and the violations of the conservative check (0).  host_only: giCDebugBlasRefitHost, the host form alone
    (no device; `differing` then counts topology bytes that left the build's, or with the same positions every byte that did)."""
    from .scene import VERTEX_DTYPE
    L = load_library()
    a = np.ascontiguousarray(vertices_a, VERTEX_DTYPE)
    b = np.ascontiguousarray(vertices_b, VERTEX_DTYPE)
    if len(a) != len(b):
        raise ValueError("debug_blas_refit: both point sets must have one entry per vertex")
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    nodes, violations = C.c_uint32(0), C.c_uint32(0)
    fn = L.giCDebugBlasRefitHost if host_only else L.giCDebugBlasRefit
    n = fn(a.ctypes.data, b.ctypes.data, len(a), f.ctypes.data, len(f), C.byref(nodes), C.byref(violations))
    if n < 0:
        raise GiError("giCDebugBlasRefit failed: " + L.giCGetLastError().decode())
    return int(n), int(nodes.value), int(violations.value)


def debug_append_records(vertices, faces, xforms, face_ids=None, max_face_id=0, flip_facing=False, double_sided=False, vertex_offset=0, shade_base=0, id_base=0,
                         mat_flags=0, host_only=False) -> int:
    """giCDebugAppendRecords: the device kernels that make an appended mesh's records on a two-level scene without the flat tree (k_append_shade_index,
    k_gather_shade, k_append_blas_tris, k_append_records) over the mesh (`vertices`: VERTEX_DTYPE, `faces`: n x 3 indices, `face_ids`: n or None) under each of
    `xforms` (k x 4 x 4, USD row vectors), laid out behind `vertex_offset` vertex records, `shade_base` shading records and the scene-order id `id_base`, against
    the scene build's own host code.  Returns the number of differing bytes (0 is the contract).  host_only: giCDebugAppendRecordsHost, the host forms of the
    same kernels (gi_append.h) against the same references (no device)."""
    from .scene import VERTEX_DTYPE
    L = load_library()
    v = np.ascontiguousarray(vertices, VERTEX_DTYPE)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    x = np.ascontiguousarray(xforms, np.float32).reshape(-1, 16)
    ids = None if face_ids is None else np.ascontiguousarray(face_ids, np.int32).reshape(-1)
    if ids is not None and len(ids) != len(f):
        raise ValueError("debug_append_records: one face id per face")
    fn = L.giCDebugAppendRecordsHost if host_only else L.giCDebugAppendRecords
    n = fn(v.ctypes.data, len(v), f.ctypes.data, len(f), None if ids is None else ids.ctypes.data, int(max_face_id), (1 if flip_facing else 0) | (2 if double_sided else 0),
           x.ctypes.data_as(_FP), len(x), int(vertex_offset), int(shade_base), int(id_base), int(mat_flags))
    if n < 0:
        raise GiError("giCDebugAppendRecords failed: " + L.giCGetLastError().decode())
    return int(n)


class _DebugInstanceMesh(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("faces", C.c_void_p), ("faceIds", C.c_void_p), ("vertexCount", C.c_uint32), ("faceCount", C.c_uint32),
                ("maxFaceId", C.c_uint32), ("flags", C.c_uint32)]


class _DebugInstanceJob(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("instanceSlot", C.c_uint32), ("recordSlot", C.c_uint32), ("idBase", C.c_uint32), ("transform", C.c_float * 16)]


def debug_instance_records(meshes, jobs, host_only=False) -> int:
    """giCDebugInstanceRecords: the device kernel that makes the flat records, face-id words and id-table words of new instances of built meshes on a two-level
    scene without the flat tree (k_instance_records, one launch for all jobs) against the scene build's own host code.  `meshes`: dicts with "vertices"
    (VERTEX_DTYPE), "faces" (n x 3) and optionally "face_ids" (n), "max_face_id", "flip_facing", "double_sided"; `jobs`: dicts with "mesh" (index), "xform"
    (4 x 4, USD row vectors), "instance_slot", "record_slot" (first flat record) and "id_base" -- slots in any order, with gaps.  Returns the number of differing
    bytes over the whole scratch arrays (0 is the contract).  host_only: giCDebugInstanceRecordsHost, the host form of the kernel (gi_instances.h) against the
    same references (no device)."""
    from .scene import VERTEX_DTYPE
    L = load_library()
    keep = []
    ms = (_DebugInstanceMesh * max(len(meshes), 1))()
    for k, m in enumerate(meshes):
        v = None if m.get("vertices") is None else np.ascontiguousarray(m["vertices"], VERTEX_DTYPE)
        f = None if m.get("faces") is None else np.ascontiguousarray(m["faces"], np.uint32).reshape(-1, 3)
        ids = None if m.get("face_ids") is None else np.ascontiguousarray(m["face_ids"], np.int32).reshape(-1)
        if ids is not None and f is not None and len(ids) != len(f):
            raise ValueError("debug_instance_records: one face id per face")
        keep += [v, f, ids]
        ms[k].vertices = None if v is None else v.ctypes.data
        ms[k].faces = None if f is None else f.ctypes.data
        ms[k].faceIds = None if ids is None else ids.ctypes.data
        ms[k].vertexCount = 0 if v is None else len(v)
        ms[k].faceCount = 0 if f is None else len(f)
        ms[k].maxFaceId = int(m.get("max_face_id", 0))
        ms[k].flags = (1 if m.get("flip_facing") else 0) | (2 if m.get("double_sided") else 0)
    js = (_DebugInstanceJob * max(len(jobs), 1))()
    for k, j in enumerate(jobs):
        js[k].mesh, js[k].instanceSlot, js[k].recordSlot, js[k].idBase = int(j["mesh"]), int(j["instance_slot"]), int(j["record_slot"]), int(j["id_base"])
        js[k].transform = (C.c_float * 16)(*np.ascontiguousarray(j["xform"], np.float32).reshape(16).tolist())
    fn = L.giCDebugInstanceRecordsHost if host_only else L.giCDebugInstanceRecords
    n = fn(C.addressof(ms) if len(meshes) else None, len(meshes), C.addressof(js) if len(jobs) else None, len(jobs))
    del keep
    if n < 0:
        raise GiError("giCDebugInstanceRecords failed: " + L.giCGetLastError().decode())
    return int(n)


class _DebugCompactRange(C.Structure):
    _fields_ = [("count", C.c_uint32), ("live", C.c_uint32), ("delta", C.c_uint32 * 3), ("hidden", C.c_uint32)]


# the array kinds of a compaction (gi_compact.h) and the bytes of one record of each
COMPACT_VERTS, COMPACT_BLAS_TRIS, COMPACT_WORDS, COMPACT_SHADE, COMPACT_BLAS_NODES, COMPACT_INSTANCES, COMPACT_INST_TRAV, COMPACT_TRIS = range(8)
COMPACT_RECORD_BYTES = {COMPACT_VERTS: 48, COMPACT_BLAS_TRIS: 64, COMPACT_WORDS: 4, COMPACT_SHADE: 160, COMPACT_BLAS_NODES: 80, COMPACT_INSTANCES: 96, COMPACT_INST_TRAV: 128,
                        COMPACT_TRIS: 64}


def debug_compact_ranges(kind, records, ranges, host_only=False):
    """giCDebugCompactRanges: the device kernel that compacts one array kind of a two-level scene (k_compact_ranges, one launch for all ranges) against a
    straightforward restatement -- filter, then rebase.  `kind`: COMPACT_*; `records`: an array whose bytes are the records (COMPACT_RECORD_BYTES[kind] each);
    `ranges`: consecutive ranges that cover them, dicts with "count", "live" and, for a live one, optionally "delta" (up to three words, by kind:
    gi_compact.h) and "hidden" (kind COMPACT_TRIS: its records do not write the id table).  Returns (differing bytes -- 0 is the contract --, info) with
    info = {"wave_items", "block_items" (whole items a wave / a workgroup holds under the mapping as built), "live", "workgroups"}.  host_only:
    giCDebugCompactRangesHost, the host form of the kernel (gi_compact.h) against the same restatement (no device)."""
    L = load_library()
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
    size = COMPACT_RECORD_BYTES[int(kind)]
    if len(raw) % size:
        raise ValueError("debug_compact_ranges: the records are not whole")
    rs = (_DebugCompactRange * max(len(ranges), 1))()
    for k, r in enumerate(ranges):
        d = [int(x) & 0xffffffff for x in r.get("delta", ())] + [0, 0, 0]
        rs[k].count, rs[k].live, rs[k].hidden = int(r["count"]), 1 if r["live"] else 0, 1 if r.get("hidden") else 0
        rs[k].delta = (C.c_uint32 * 3)(*d[:3])
    info = (C.c_uint32 * 4)()
    fn = L.giCDebugCompactRangesHost if host_only else L.giCDebugCompactRanges
    n = fn(int(kind), raw.ctypes.data if len(raw) else None, len(raw) // size, C.addressof(rs) if len(ranges) else None, len(ranges), info)
    if n < 0:
        raise GiError("giCDebugCompactRanges failed: " + L.giCGetLastError().decode())
    return int(n), {"wave_items": int(info[0]), "block_items": int(info[1]), "live": int(info[2]), "workgroups": int(info[3])}


def debug_patch_visibility_two_level(face_counts, hidden_before, hidden_after, seed=1):
    """giCDebugPatchVisibilityTwoLevel: the device kernels of a visibility update of the two-level layout (k_patch_visibility2 / k_patch_inst_trav) over
    synthetic records -- one instance per entry in scene order with `face_counts[i]` triangles, hidden before / after the edit where the flags say so, laid
    out in a shuffled flat order drawn from `seed` -- against the host form of the same code, and the host form against a fresh numbering.  Returns
    (differing, triangles): the words of TriRec::origId, the id table and InstTrav::triBase that differ, plus the host form's violations (0 is the contract),
    and the resident triangles.  Needs an initialised device."""
    L = load_library()
    n = np.ascontiguousarray(face_counts, np.uint32)
    hb = np.ascontiguousarray(hidden_before, np.uint8)
    ha = np.ascontiguousarray(hidden_after, np.uint8)
    if not (len(n) == len(hb) == len(ha)):
        raise ValueError("debug_patch_visibility_two_level: one entry per instance in all three arrays")
    tris = C.c_uint32(0)
    v = L.giCDebugPatchVisibilityTwoLevel(n.ctypes.data_as(C.POINTER(C.c_uint32)), hb.ctypes.data_as(C.POINTER(C.c_uint8)), ha.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          len(n), int(seed), C.byref(tris))
    if v < 0:
        raise GiError("giCDebugPatchVisibilityTwoLevel failed: " + L.giCGetLastError().decode())
    return int(v), int(tris.value)


class FlatIdCheck(int):
    """Scene.flat_id_check's answer: the number of violations as an int, with what the hook reports beside it."""
    visible_tris = 0
    resident_tris = 0
    hidden_instances = 0
    two_level = 0


class BlasCheck(int):
    """Scene.blas_check's answer: differences plus conservative violations as an int, with what the hook reports beside it."""
    two_level = 0
    blas_nodes = 0
    violations = 0
    blas_tris = 0


class TlasCheck(int):
    """Scene.tlas_check's answer: the number of differing records as an int, with what the hook reports beside it."""
    two_level = 0
    instances = 0
    tlas_nodes = 0
    tlas_depth = 0


_initialized = False


def initialize(device: int = 0, devices=None):
    """One giCInitialize per process (Gi.cpp:244-259).  `devices` = list of HIP ordinals -> giCInitializeDevices: whole-frame renders are then dealt
    row-wise to all of them inside the library (the first is the primary); $GATLING_DEVICES does the same for callers that pass nothing."""
    global _initialized
    L = load_library()
    if not _initialized:
        if devices:
            arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            rc = L.giCInitializeDevices(arr, len(devices))
        else:
            rc = L.giCInitialize(device)
        if rc != GI_C_OK:
            raise GiError("giCInitialize failed: " + L.giCGetLastError().decode())
        _initialized = True
    return L


def _camera(cam) -> GiCCameraDesc:
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    return GiCCameraDesc(f3(cam.position), f3(cam.forward), f3(cam.up), cam.vfov, cam.f_stop, cam.focus_distance,
                         cam.focal_length, cam.clip_start, cam.clip_end, cam.exposure)


def _settings(rs: RenderSettings) -> GiCRenderSettings:
    s = GiCRenderSettings()
    s.clippingPlanes = int(rs.clipping_planes); s.depthOfField = int(rs.depth_of_field)
    s.domeLightCameraVisible = int(rs.dome_light_camera_visible); s.filterImportanceSampling = int(rs.filter_importance_sampling)
    s.frame = float(getattr(rs, "frame", 0.0)); s.jitteredSampling = int(rs.jittered_sampling); s.lightIntensityMultiplier = rs.light_intensity_multiplier
    s.maxBounces = rs.max_bounces; s.maxSampleValue = rs.max_sample_value; s.maxVolumeWalkLength = rs.max_volume_walk_length
    s.mediumStackSize = rs.medium_stack_size; s.metersPerSceneUnit = rs.meters_per_scene_unit
    s.nextEventEstimation = int(rs.next_event_estimation); s.progressiveAccumulation = int(rs.progressive_accumulation)
    s.rrBounceOffset = rs.rr_bounce_offset; s.rrInvMinTermProb = rs.rr_inv_min_term_prob; s.spp = rs.spp; s.time = 0.0
    return s


class Scene:
    """Feeds a :class:`SceneDesc` through the gi C ABI the way hdGatling feeds Hydra prims through Gi.h."""

    def __init__(self, desc: SceneDesc, device: int = 0, mtlx_materials=None):
        """`mtlx_materials`: {material index: MaterialX document string} -- those materials are created through the gtl shim's MaterialX reader
        (gtl::giCreateMaterialFromMtlxStr, what hdGatling calls) instead of giCCreateMaterial with the parameter block."""
        self.L = initialize(device)
        L = self.L
        self.desc = desc
        self.handle = L.giCCreateScene()
        if not self.handle:
            raise GiError("giCCreateScene failed")
        self.materials, self.meshes, self.lights, self.textures, self.dome = [], [], [], [], None
        for t in getattr(desc, "textures", []):
            a = np.ascontiguousarray(t, np.float32)
            td = GiCTextureDesc(a.shape[1], a.shape[0], a.ctypes.data)
            h = L.giCCreateTexture(self.handle, C.byref(td))  # copies the pixels
            if not h:
                raise GiError("giCCreateTexture failed: " + L.giCGetLastError().decode())
            self.textures.append(h)
        for mi, m in enumerate(desc.materials):
            if mtlx_materials and mi in mtlx_materials:
                L.gtlCreateMaterialFromMtlxStrC.restype = C.c_void_p
                L.gtlCreateMaterialFromMtlxStrC.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
                h = L.gtlCreateMaterialFromMtlxStrC(self.handle, m.name.encode(), mtlx_materials[mi].encode())
                if not h:
                    raise GiError("gtl::giCreateMaterialFromMtlxStr refused the document of material %d" % mi)
                self.materials.append(h)
                continue
            h = self._material_handle(m)
            self.materials.append(h)
        if getattr(desc, "dome_light", None) is not None:
            d = desc.dome_light
            self.dome = L.giCCreateDomeLight(self.handle, b"")
            if d.texture >= 0:
                L.giCSetDomeLightTexture(self.dome, self.textures[d.texture])
            L.giCSetDomeLightRotation(self.dome, _fp(d.rotation)); L.giCSetDomeLightBaseEmission(self.dome, _fp(d.base_emission))
            L.giCSetDomeLightDiffuseSpecular(self.dome, d.diffuse, d.specular)
        for m in desc.meshes:
            self.meshes.append(self._mesh_handle(m))
        for l in desc.sphere_lights:
            h = L.giCCreateSphereLight(self.handle)
            L.giCSetSphereLightPosition(h, _fp(l.pos)); L.giCSetSphereLightBaseEmission(h, _fp(l.base_emission))
            L.giCSetSphereLightRadius(h, *[float(x) for x in l.radius]); L.giCSetSphereLightDiffuseSpecular(h, l.diffuse, l.specular)
            self.lights.append(("sphere", h))
        for l in desc.distant_lights:
            h = L.giCCreateDistantLight(self.handle)
            L.giCSetDistantLightDirection(h, _fp(l.direction)); L.giCSetDistantLightBaseEmission(h, _fp(l.base_emission))
            L.giCSetDistantLightAngle(h, l.angle); L.giCSetDistantLightDiffuseSpecular(h, l.diffuse, l.specular)
            self.lights.append(("distant", h))
        for l in desc.rect_lights:
            h = L.giCCreateRectLight(self.handle)
            L.giCSetRectLightOrigin(h, _fp(l.origin)); L.giCSetRectLightTangents(h, _fp(l.t0), _fp(l.t1))
            L.giCSetRectLightBaseEmission(h, _fp(l.base_emission)); L.giCSetRectLightDimensions(h, l.width, l.height)
            L.giCSetRectLightDiffuseSpecular(h, l.diffuse, l.specular)
            self.lights.append(("rect", h))
        for l in desc.disk_lights:
            h = L.giCCreateDiskLight(self.handle)
            L.giCSetDiskLightOrigin(h, _fp(l.origin)); L.giCSetDiskLightTangents(h, _fp(l.t0), _fp(l.t1))
            L.giCSetDiskLightBaseEmission(h, _fp(l.base_emission)); L.giCSetDiskLightRadius(h, l.radius_x, l.radius_y)
            L.giCSetDiskLightDiffuseSpecular(h, l.diffuse, l.specular)
            self.lights.append(("disk", h))
        self._buffers = {}

    def _mesh_handle(self, m):
        """giCCreateMesh and the setters hdGatling runs on every new mesh (mesh.cpp _CreateGiMeshes + Sync: transform, instance transforms, instance ids,
        primvars, instancer primvars, material, visibility) for one MeshDesc."""
        L = self.L
        v = np.ascontiguousarray(m.vertices)
        f = np.ascontiguousarray(m.faces, np.uint32)
        fid = np.ascontiguousarray(m.face_ids, np.int32) if m.face_ids is not None else None
        d = GiCMeshDesc(len(f), f.ctypes.data, fid.ctypes.data if fid is not None else None, m.id, int(m.double_sided),
                        int(m.left_handed), m.name.encode(), int(m.max_face_id), len(v), v.ctypes.data)
        h = L.giCCreateMesh(self.handle, C.byref(d))
        if not h:
            raise GiError("giCCreateMesh failed: " + L.giCGetLastError().decode())
        L.giCSetMeshTransform(h, _fp(np.asarray(m.transform, np.float32).reshape(-1)))
        it = np.ascontiguousarray(m.instance_transforms, np.float32).reshape(-1, 16)
        L.giCSetMeshInstanceTransforms(h, len(it), it.ctypes.data_as(_FP))
        if m.instance_ids is not None:
            ids = np.ascontiguousarray(m.instance_ids, np.int32)
            L.giCSetMeshInstanceIds(h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int32)))
        for attr, fn in (("primvars", L.giCSetMeshPrimvars), ("instancer_primvars", L.giCSetMeshInstancerPrimvars)):
            pvs = getattr(m, attr, [])
            if pvs:
                arr, keep = (GiCPrimvarData * len(pvs))(), []
                for k, pv in enumerate(pvs):
                    d = np.ascontiguousarray(pv.data, np.int32 if int(pv.type) >= 4 else np.float32).reshape(-1)  # Int..Int4 (Gi.h:76-79)
                    keep.append(d)
                    arr[k] = GiCPrimvarData(pv.name.encode(), int(pv.type), int(pv.interpolation), d.ctypes.data, d.nbytes)
                if fn(h, len(pvs), arr) != GI_C_OK:  # copies the data
                    raise GiError("giCSetMesh*Primvars failed: " + L.giCGetLastError().decode())
        if m.material >= 0:
            L.giCSetMeshMaterial(h, self.materials[m.material])
        L.giCSetMeshVisibility(h, int(m.visible))
        return h

    def create_mesh(self, mesh_desc) -> int:
        """giCCreateMesh on a live scene with every setter hdGatling runs on a new mesh; the mesh is appended to desc.meshes.  Returns its index.  A topology
        edit: the next render rebuilds the scene -- or, with OPTION_TOPOLOGY_UPDATES, appends the mesh to the resident scene."""
        self.meshes.append(self._mesh_handle(mesh_desc))
        self.desc.meshes.append(mesh_desc)
        return len(self.meshes) - 1

    def destroy_mesh(self, mesh_index: int):
        """giCDestroyMesh on a live scene; the entry leaves desc.meshes too (later indices shift down), so desc stays the description a fresh build sees."""
        self.L.giCDestroyMesh(self.meshes.pop(mesh_index))
        del self.desc.meshes[mesh_index]

    def topology_update_count(self) -> int:
        """giCDebugSceneTopologyUpdateCount: how often the scene was brought up to date by an incremental topology update (not counted by update_counts)."""
        n = C.c_uint64(0)
        if self.L.giCDebugSceneTopologyUpdateCount(self.handle, C.byref(n)) != GI_C_OK:
            raise GiError("giCDebugSceneTopologyUpdateCount failed")
        return int(n.value)

    def tlas_update_count(self) -> int:
        """giCDebugSceneTlasUpdateCount: how often the scene was brought up to date by a transform update of the two-level layout (OPTION_TLAS_UPDATES; not
        counted by update_counts)."""
        n = C.c_uint64(0)
        if self.L.giCDebugSceneTlasUpdateCount(self.handle, C.byref(n)) != GI_C_OK:
            raise GiError("giCDebugSceneTlasUpdateCount failed")
        return int(n.value)

    def blas_update_count(self) -> int:
        """giCDebugSceneBlasUpdateCount: how often the scene was brought up to date by a vertex update of the two-level layout (OPTION_BLAS_UPDATES; counted
        neither in update_counts() nor in vertex_update_count())."""
        n = C.c_uint64(0)
        if self.L.giCDebugSceneBlasUpdateCount(self.handle, C.byref(n)) != GI_C_OK:
            raise GiError("giCDebugSceneBlasUpdateCount failed")
        return int(n.value)

    def tlas_visibility_update_count(self) -> int:
        """giCDebugSceneTlasVisibilityUpdateCount: how often the scene was brought up to date by a visibility update of the two-level layout
        (OPTION_TLAS_VISIBILITY; counted neither in update_counts() nor in visibility_update_count())."""
        n = C.c_uint64(0)
        if self.L.giCDebugSceneTlasVisibilityUpdateCount(self.handle, C.byref(n)) != GI_C_OK:
            raise GiError("giCDebugSceneTlasVisibilityUpdateCount failed")
        return int(n.value)

    def tlas_topology_update_count(self) -> int:
        """giCDebugSceneTlasTopologyUpdateCount: how often the scene was brought up to date by a topology update of the two-level layout
        (OPTION_TLAS_TOPOLOGY; counted neither in update_counts() nor in topology_update_count())."""
        n = C.c_uint64(0)
        if self.L.giCDebugSceneTlasTopologyUpdateCount(self.handle, C.byref(n)) != GI_C_OK:
            raise GiError("giCDebugSceneTlasTopologyUpdateCount failed")
        return int(n.value)

    def tlas_instance_update_stats(self) -> dict:
        """giCDebugSceneTlasInstanceUpdateStats: instancer edits applied in place on the two-level layout (OPTION_TLAS_INSTANCES).  Returns {"syncs",
        "appended", "reused" (of the appended instances, how many went into the storage slots retired ones left), "retired"}.  Such a sync counts once in
        tlas_topology_update_count(), and neither in update_counts() nor in instance_update_count()."""
        out = (C.c_uint64 * 4)()
        if self.L.giCDebugSceneTlasInstanceUpdateStats(self.handle, out) != GI_C_OK:
            raise GiError("giCDebugSceneTlasInstanceUpdateStats failed")
        return {"syncs": int(out[0]), "appended": int(out[1]), "reused": int(out[2]), "retired": int(out[3])}

    def compaction_stats(self) -> dict:
        """giCDebugSceneCompactionCount: compactions of the retired ranges of this scene (OPTION_TLAS_COMPACTION).  Returns {"applied", "records_moved",
        "bytes_released" (on the primary device), "declined"}.  A compaction is part of the sync that triggers it: it has no entry in update_counts()."""
        out = (C.c_uint64 * 4)()
        if self.L.giCDebugSceneCompactionCount(self.handle, out) != GI_C_OK:
            raise GiError("giCDebugSceneCompactionCount failed")
        return {"applied": int(out[0]), "records_moved": int(out[1]), "bytes_released": int(out[2]), "declined": int(out[3])}

    def compaction_count(self) -> int:
        """Compactions applied to this scene (compaction_stats()["applied"])."""
        return self.compaction_stats()["applied"]

    def tlas_build_stats(self) -> dict:
        """giCDebugSceneTlasBuildStats: the TLAS builds of edits in place under OPTION_TLAS_DEVICE_BUILD.  Returns {"device_builds", "too_deep", "out_of_memory",
        "error", "under_min" (the four fallbacks to the host builder), "stage_us" (upload + boxes + sort, PLOC, emission, read-back of the last device build),
        "passes", "host_waits", "depth", "nodes", "allocations", "resident_device_built", "budget"}.  All zero with the option off."""
        out = (C.c_uint64 * 16)()
        if self.L.giCDebugSceneTlasBuildStats(self.handle, out) != GI_C_OK:
            raise GiError("giCDebugSceneTlasBuildStats failed")
        return {"device_builds": int(out[0]), "too_deep": int(out[1]), "out_of_memory": int(out[2]), "error": int(out[3]), "under_min": int(out[4]),
                "stage_us": [int(out[5 + k]) for k in range(4)], "passes": int(out[9]), "host_waits": int(out[10]), "depth": int(out[11]), "nodes": int(out[12]),
                "allocations": int(out[13]), "resident_device_built": int(out[14]), "budget": int(out[15])}

    def blas_build_stats(self) -> dict:
        """giCDebugSceneBlasBuildStats: the BLAS builds of this scene under OPTION_BLAS_DEVICE_BUILD.  Returns {"device_builds", "under_min", "over_max", "too_deep",
        "out_of_memory", "error" (the five fallbacks to the host builder), "stage_us" (upload + face boxes + sort, PLOC, emission, read-back of the last device
        build), "passes", "host_waits", "depth", "nodes", "budget", "resident_device_built" (meshes of the resident scene)}.  All zero with the option off."""
        out = (C.c_uint64 * 16)()
        if self.L.giCDebugSceneBlasBuildStats(self.handle, out) != GI_C_OK:
            raise GiError("giCDebugSceneBlasBuildStats failed")
        return {"device_builds": int(out[0]), "under_min": int(out[1]), "over_max": int(out[2]), "too_deep": int(out[3]), "out_of_memory": int(out[4]),
                "error": int(out[5]), "stage_us": [int(out[6 + k]) for k in range(4)], "passes": int(out[10]), "host_waits": int(out[11]), "depth": int(out[12]),
                "nodes": int(out[13]), "budget": int(out[14]), "resident_device_built": int(out[15])}

    def flat_id_check(self, device: int = 0) -> "FlatIdCheck":
        """giCDebugSceneFlatIdCheck: the flat records, the id table and the per-instance records resident on a device -- the ids of visible records are a
        permutation of [0, visible), the table names each at its id, triBase + prim is the id, hidden records have zero edges.  Returns the violations (0) as a
        FlatIdCheck: .visible_tris, .resident_tris, .hidden_instances, .two_level (1 when the layout is in use; 0: nothing was compared)."""
        out = (C.c_uint32 * 4)()
        v = self.L.giCDebugSceneFlatIdCheck(self.handle, device, out)
        if v < 0:
            raise GiError("giCDebugSceneFlatIdCheck failed: " + self.L.giCGetLastError().decode())
        r = FlatIdCheck(v)
        r.visible_tris, r.resident_tris, r.hidden_instances, r.two_level = int(out[0]), int(out[1]), int(out[2]), int(out[3])
        return r

    def flat_tree_state(self, device: int = 0) -> dict:
        """giCDebugSceneFlatTreeState: what a scene rendered at least once holds of the flat tree (OPTION_TLAS_ONLY).  Returns {"two_level", "treeless" (1: built
        without the flat tree), "resident_nodes" (flat nodes on `device`), "host_node_bytes"}."""
        out = (C.c_uint64 * 4)()
        if self.L.giCDebugSceneFlatTreeState(self.handle, device, out) != GI_C_OK:
            raise GiError("giCDebugSceneFlatTreeState failed: " + self.L.giCGetLastError().decode())
        return {"two_level": int(out[0]), "treeless": int(out[1]), "resident_nodes": int(out[2]), "host_node_bytes": int(out[3])}

    def blas_check(self, device: int = 0) -> "BlasCheck":
        """giCDebugSceneBlasCheck: the two-level arrays resident on a device against the current meshes after vertex updates in place -- BLAS triangles, BLAS
        nodes against the host form of the refit, TLAS, items and per-instance records against a fresh build.  Returns differences + conservative violations
        (0) as a BlasCheck: .two_level (1 when the layout is in use), .blas_nodes, .violations (the conservative check alone), .blas_tris."""
        out = (C.c_uint32 * 4)()
        v = self.L.giCDebugSceneBlasCheck(self.handle, device, out)
        if v < 0:
            raise GiError("giCDebugSceneBlasCheck failed: " + self.L.giCGetLastError().decode())
        r = BlasCheck(v)
        r.two_level, r.blas_nodes, r.violations, r.blas_tris = int(out[0]), int(out[1]), int(out[2]), int(out[3])
        return r

    def tlas_check(self, device: int = 0) -> "TlasCheck":
        """giCDebugSceneTlasCheck: the two-level arrays resident on a device against the arrays the scene build's code makes anew from the current meshes.
        Returns the number of differing records (0) as a TlasCheck: .two_level (1 when the layout is in use), .instances, .tlas_nodes, .tlas_depth."""
        out = (C.c_uint32 * 4)()
        v = self.L.giCDebugSceneTlasCheck(self.handle, device, out)
        if v < 0:
            raise GiError("giCDebugSceneTlasCheck failed: " + self.L.giCGetLastError().decode())
        r = TlasCheck(v)
        r.two_level, r.instances, r.tlas_nodes, r.tlas_depth = int(out[0]), int(out[1]), int(out[2]), int(out[3])
        return r

    def set_mesh_transform(self, mesh_index: int, matrix):
        """giSetMeshTransform (Gi.h:213): a transform-only edit -- the next render updates the scene incrementally."""
        m = np.ascontiguousarray(matrix, np.float32).reshape(16)
        self.desc.meshes[mesh_index].transform = m.reshape(4, 4).copy()
        self.L.giCSetMeshTransform(self.meshes[mesh_index], m.ctypes.data_as(_FP))

    def set_mesh_instance_transforms(self, mesh_index: int, transforms):
        """giSetMeshInstanceTransforms (Gi.h:214)."""
        t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 16)
        self.desc.meshes[mesh_index].instance_transforms = t.reshape(-1, 4, 4).copy()
        self.L.giCSetMeshInstanceTransforms(self.meshes[mesh_index], len(t), t.ctypes.data_as(_FP))

    def set_mesh_instance_ids(self, mesh_index: int, ids):
        """giSetMeshInstanceIds (Gi.h:215).  On a built mesh the next render rebuilds the scene -- or, with OPTION_INSTANCE_UPDATES, re-sends the instance records."""
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        self.desc.meshes[mesh_index].instance_ids = a.copy()
        self.L.giCSetMeshInstanceIds(self.meshes[mesh_index], len(a), a.ctypes.data_as(C.POINTER(C.c_int32)))

    def instance_update_counts(self) -> dict:
        """giCDebugSceneInstanceUpdateCount: syncs that applied an instancer edit in place, instances appended, of those cloned on the device, instances retired."""
        c = (C.c_uint64 * 4)()
        if self.L.giCDebugSceneInstanceUpdateCount(self.handle, c) != GI_C_OK:
            raise GiError("giCDebugSceneInstanceUpdateCount failed")
        return {"syncs": int(c[0]), "appended": int(c[1]), "cloned": int(c[2]), "retired": int(c[3])}

    def _material_handle(self, m):
        """giCCreateMaterial + texture bindings + primvar inputs of one MaterialDesc (texture indices name self.textures)."""
        L = self.L
        md = GiCMaterialDesc(m.klass, 0, (C.c_float * P_COUNT)(*np.asarray(m.params, np.float32)))
        h = L.giCCreateMaterial(self.handle, m.name.encode(), C.byref(md))
        if not h:
            raise GiError("giCCreateMaterial failed: " + L.giCGetLastError().decode())
        for slot, b in getattr(m, "textures", {}).items():
            self._bind_texture(h, slot, b)
        for slot, name in getattr(m, "primvar_inputs", {}).items():
            if L.giCSetMaterialPrimvarInput(h, int(slot), name.encode()) != GI_C_OK:
                raise GiError("giCSetMaterialPrimvarInput failed: " + L.giCGetLastError().decode())
        return h

    def _bind_texture(self, h, slot, b):
        L = self.L
        tb = GiCTextureBinding(self.textures[b.texture], int(b.wrap_s), int(b.wrap_t), int(b.channel), (C.c_float * 4)(*b.scale), (C.c_float * 4)(*b.bias))
        if L.giCSetMaterialTexture(h, int(slot), C.byref(tb)) != GI_C_OK:
            raise GiError("giCSetMaterialTexture failed: " + L.giCGetLastError().decode())
        if L.giCSetMaterialTextureTransform(h, int(slot), _fp(b.transform) if getattr(b, "transform", None) is not None else None) != GI_C_OK:
            raise GiError("giCSetMaterialTextureTransform failed: " + L.giCGetLastError().decode())

    def set_mesh_material(self, mesh_index: int, material_index: int):
        """giSetMeshMaterial (Gi.h:215); material_index < 0 = NULL (the mesh drops out of the scene).  A material-side edit: the next render patches the scene
        in place."""
        self.desc.meshes[mesh_index].material = int(material_index)
        self.L.giCSetMeshMaterial(self.meshes[mesh_index], self.materials[material_index] if material_index >= 0 else None)

    def replace_material(self, material_index: int, desc):
        """Edits a material the way hdGatling does: destroy it, create the new one, re-assign the meshes that were bound to it."""
        self.L.giCDestroyMaterial(self.materials[material_index])
        self.materials[material_index] = None
        self.materials[material_index] = self._material_handle(desc)
        self.desc.materials[material_index] = desc
        for i, m in enumerate(self.desc.meshes):
            if m.material == material_index:
                self.L.giCSetMeshMaterial(self.meshes[i], self.materials[material_index])

    def destroy_material(self, material_index: int):
        """giDestroyMaterial alone: the meshes bound to it are left without a material (and out of the scene) until they get another."""
        self.L.giCDestroyMaterial(self.materials[material_index])
        self.materials[material_index] = None

    def set_material_texture(self, material_index: int, slot: int, binding):
        """giCSetMaterialTexture on a live material; binding None unbinds the input."""
        m = self.desc.materials[material_index]
        if binding is None:
            m.textures.pop(slot, None)
            if self.L.giCSetMaterialTexture(self.materials[material_index], int(slot), None) != GI_C_OK:
                raise GiError("giCSetMaterialTexture failed: " + self.L.giCGetLastError().decode())
        else:
            m.textures[slot] = binding
            self._bind_texture(self.materials[material_index], slot, binding)

    def add_texture(self, image) -> int:
        """giCCreateTexture on a live scene; returns the index into desc.textures."""
        a = np.ascontiguousarray(image, np.float32)
        td = GiCTextureDesc(a.shape[1], a.shape[0], a.ctypes.data)
        h = self.L.giCCreateTexture(self.handle, C.byref(td))
        if not h:
            raise GiError("giCCreateTexture failed: " + self.L.giCGetLastError().decode())
        self.textures.append(h); self.desc.textures.append(a)
        return len(self.textures) - 1

    def set_material_primvar_input(self, material_index: int, slot: int, name):
        """giCSetMaterialPrimvarInput on a live material; name None / "" disconnects the input."""
        m = self.desc.materials[material_index]
        if name:
            m.primvar_inputs[slot] = name
        else:
            m.primvar_inputs.pop(slot, None)
        if self.L.giCSetMaterialPrimvarInput(self.materials[material_index], int(slot), name.encode() if name else None) != GI_C_OK:
            raise GiError("giCSetMaterialPrimvarInput failed: " + self.L.giCGetLastError().decode())

    def _set_primvars(self, fn, h, pvs):
        arr, keep = (GiCPrimvarData * max(len(pvs), 1))(), []
        for k, pv in enumerate(pvs):
            d = np.ascontiguousarray(pv.data, np.int32 if int(pv.type) >= 4 else np.float32).reshape(-1)  # Int..Int4 (Gi.h:76-79)
            keep.append(d)
            arr[k] = GiCPrimvarData(pv.name.encode(), int(pv.type), int(pv.interpolation), d.ctypes.data, d.nbytes)
        if fn(h, len(pvs), arr) != GI_C_OK:  # copies the data
            raise GiError("giCSetMesh*Primvars failed: " + self.L.giCGetLastError().decode())

    def set_mesh_primvars(self, mesh_index: int, primvars):
        """giCSetMeshPrimvars on a live mesh (replaces the mesh's primvar list)."""
        self.desc.meshes[mesh_index].primvars = list(primvars)
        self._set_primvars(self.L.giCSetMeshPrimvars, self.meshes[mesh_index], list(primvars))

    def set_mesh_instancer_primvars(self, mesh_index: int, primvars):
        self.desc.meshes[mesh_index].instancer_primvars = list(primvars)
        self._set_primvars(self.L.giCSetMeshInstancerPrimvars, self.meshes[mesh_index], list(primvars))

    def set_mesh_visibility(self, mesh_index: int, visible: bool):
        """giSetMeshVisibility (Gi.h:216): a geometry-side edit, the next render rebuilds the scene -- or, with OPTION_VISIBILITY_UPDATES, updates it in place."""
        self.desc.meshes[mesh_index].visible = bool(visible)
        self.L.giCSetMeshVisibility(self.meshes[mesh_index], int(bool(visible)))

    def set_mesh_vertices(self, mesh_index: int, vertices):
        """giCSetMeshVertices: the mesh's vertex array replaced (same count; faces, ids, primvars, material and transforms stay).  A geometry-side edit: the
        next render rebuilds the scene -- or, with OPTION_VERTEX_UPDATES, refits the resident BVH on the device.  A refused array leaves the mesh unchanged."""
        from .scene import VERTEX_DTYPE
        v = np.ascontiguousarray(vertices, VERTEX_DTYPE)
        if self.L.giCSetMeshVertices(self.meshes[mesh_index], len(v), v.ctypes.data) != GI_C_OK:
            raise GiError("giCSetMeshVertices failed: " + self.L.giCGetLastError().decode())
        self.desc.meshes[mesh_index].vertices = v.copy()

    def vertex_update_count(self) -> int:
        """giCDebugSceneVertexUpdateCount: how often the scene was brought up to date by an incremental vertex update (not counted by update_counts)."""
        n = C.c_uint64(0)
        if self.L.giCDebugSceneVertexUpdateCount(self.handle, C.byref(n)) != GI_C_OK:
            raise GiError("giCDebugSceneVertexUpdateCount failed")
        return int(n.value)

    def refit_check(self, device: int = 0) -> dict:
        """giCDebugSceneRefitCheck: the resident tree against the host's refit of it.  Returns {"differing", "nodes"}."""
        nodes = C.c_uint32(0)
        v = self.L.giCDebugSceneRefitCheck(self.handle, device, C.byref(nodes))
        if v < 0:
            raise GiError("giCDebugSceneRefitCheck failed: " + self.L.giCGetLastError().decode())
        return {"differing": v, "nodes": nodes.value}

    def shade_check(self, device: int = 0) -> int:
        """giCDebugSceneShadeCheck: the vertex and shading records resident on a device against the host's copies, whole arrays.  Returns the number of
        differing records (0)."""
        records = C.c_uint32(0)
        v = self.L.giCDebugSceneShadeCheck(self.handle, device, C.byref(records))
        if v < 0:
            raise GiError("giCDebugSceneShadeCheck failed: " + self.L.giCGetLastError().decode())
        return int(v)

    def resync_count(self) -> int:
        """giCDebugSceneResyncCount: meshes that adopted the resident records of the mesh they replaced (OPTION_RESYNC_REFITS) since the scene was created."""
        n = C.c_uint64(0)
        if self.L.giCDebugSceneResyncCount(self.handle, C.byref(n)) != GI_C_OK:
            raise GiError("giCDebugSceneResyncCount failed")
        return int(n.value)

    def update_counts(self) -> dict:
        """giCDebugSceneUpdateCounts: how often the scene was brought up to date by a full build / a transform update / a material update."""
        c = (C.c_uint64 * 3)()
        if self.L.giCDebugSceneUpdateCounts(self.handle, c) != GI_C_OK:
            raise GiError("giCDebugSceneUpdateCounts failed")
        return {"full": int(c[0]), "transform": int(c[1]), "material": int(c[2])}

    def visibility_update_count(self) -> int:
        """giCDebugSceneVisibilityUpdateCount: how often the scene was brought up to date by an incremental visibility update (not counted by update_counts)."""
        n = C.c_uint64(0)
        if self.L.giCDebugSceneVisibilityUpdateCount(self.handle, C.byref(n)) != GI_C_OK:
            raise GiError("giCDebugSceneVisibilityUpdateCount failed")
        return int(n.value)

    def class_state(self) -> dict:
        """giCDebugSceneClassState: the class masks and the cutout flag the last scene sync derived (they pick a render's kernel variants)."""
        c = (C.c_uint32 * 5)()
        if self.L.giCDebugSceneClassState(self.handle, c) != GI_C_OK:
            raise GiError("giCDebugSceneClassState failed")
        return {"classMask": int(c[0]), "classTextured": int(c[1]), "shadeClassMask": int(c[2]), "shadeClassTextured": int(c[3]), "hasCutouts": bool(c[4])}

    def ups_plain(self) -> dict:
        """giCDebugSceneUpsPlain: `traits` -- what the UsdPreviewSurface materials of the visible meshes have in common (UPS_NOCOAT) as the last scene
        sync derived it -- and `launched`, the traits the fused kernel of the last render was compiled for (0: the general kernel, or none)."""
        c = (C.c_uint32 * 2)()
        if self.L.giCDebugSceneUpsPlain(self.handle, c) != GI_C_OK:
            raise GiError("giCDebugSceneUpsPlain failed")
        return {"traits": int(c[0]), "launched": int(c[1])}

    def node_cook(self) -> bool:
        """giCDebugSceneNodeCook: whether the fused kernel of the last render staged its nodes cooked (GATLING_OPTIONS node_cook; False: the kernel that
        decodes the meta bytes ran, or no fused kernel)."""
        c = (C.c_uint32 * 1)()
        if self.L.giCDebugSceneNodeCook(self.handle, c) != GI_C_OK:
            raise GiError("giCDebugSceneNodeCook failed")
        return bool(c[0])

    def leaf_lift(self) -> dict:
        """giCDebugSceneLeafLift: `lifted` -- the leaf slots the last scene build moved into free slots of the root (OPTION_LEAF_LIFT; 0: switched off, a scene
        outside the pass, or nothing to gain) -- and `depth`, the levels of the host-built flat tree."""
        c = (C.c_uint32 * 2)()
        if self.L.giCDebugSceneLeafLift(self.handle, c) != GI_C_OK:
            raise GiError("giCDebugSceneLeafLift failed")
        return {"lifted": int(c[0]), "depth": int(c[1])}

    def path_walk_stats(self) -> dict:
        """giCDebugPathWalkStats: the fused kernel's trips and walk-step tables of the last render (OPTION_COUNT_TRAVERSAL; all zero otherwise).  stepTrips[k] /
        stepLanes[k]: trips whose closest-hit loop reached step k (7: that and every later step) and the lanes walking then; fewLaneSteps: steps begun with
        fewer than 8 lanes walking."""
        c = (C.c_uint64 * 18)()
        if self.L.giCDebugPathWalkStats(self.handle, c) != GI_C_OK:
            raise GiError("giCDebugPathWalkStats failed")
        return {"phaseTrips": int(c[0]), "stepTrips": [int(v) for v in c[1:9]], "stepLanes": [int(v) for v in c[9:17]], "fewLaneSteps": int(c[17])}

    def path_lobe_stats(self) -> dict:
        """giCDebugPathLobeStats: the fused kernel's glossy-lobe counters of the last render (OPTION_COUNT_TRAVERSAL; all zero otherwise) and, with
        GATLING_OPTIONS lobe_park set explicitly, what the lobe parking did."""
        c = (C.c_uint64 * 9)()
        if self.L.giCDebugPathLobeStats(self.handle, c) != GI_C_OK:
            raise GiError("giCDebugPathLobeStats failed")
        keys = ("shaded", "glossy", "glossyTrips", "liteTrips", "fullTrips", "parked", "adopted", "reruns", "rerunHits")
        return {k: int(v) for k, v in zip(keys, c)}

    def path_ring_stats(self) -> dict:
        """giCDebugPathRingStats: the triangle-ring counters of the fused kernel's closest-hit loops in the last render (OPTION_COUNT_TRAVERSAL; all zero
        otherwise).  With GATLING_OPTIONS ring_carry=1 set explicitly the ring is carried across the steps of a trip and flushed once at the loop's end."""
        c = (C.c_uint64 * 5)()
        if self.L.giCDebugPathRingStats(self.handle, c) != GI_C_OK:
            raise GiError("giCDebugPathRingStats failed")
        keys = ("batches", "pairs", "partialBatches", "flushes", "ballotSteps")
        return {k: int(v) for k, v in zip(keys, c)}

    def traversal_stack_high(self) -> dict:
        """giCDebugTraversalStackHigh: the most traversal-stack entries a closest-hit walk (`closest`) and a shadow walk (`shadow`) held in the last render
        (OPTION_COUNT_TRAVERSAL; all zero otherwise), the stack `rows` of the kernel variant that ran and the scratch-`spill` entries used at most (both derived on the host from the dispatch rule, not
        counted).  The primary device's walks only."""
        c = (C.c_uint32 * 4)()
        if self.L.giCDebugTraversalStackHigh(self.handle, c) != GI_C_OK:
            raise GiError("giCDebugTraversalStackHigh failed")
        return {k: int(v) for k, v in zip(("closest", "shadow", "rows", "spill"), c)}

    def set_option(self, option: int, value: int):
        if self.L.giCSetSceneOption(self.handle, option, value) != GI_C_OK:
            raise GiError("giCSetSceneOption failed")

    def color_buffer(self, width, height):
        key = ("color", width, height)
        if key not in self._buffers:
            rb = self.L.giCCreateRenderBuffer(width, height, FORMAT_FLOAT32_VEC4)
            if not rb:
                raise GiError("giCCreateRenderBuffer failed: " + self.L.giCGetLastError().decode())
            self._buffers[key] = rb
        return self._buffers[key]

    def render(self, settings: RenderSettings, width: int, height: int, rows=None, device_only=False, row_stride=1, copy=True):
        """One giCRender call.  Returns the colour AOV as float32 [rows, width, 4] (row 0 = bottom) -- the library-owned host
        memory of giCGetRenderBufferMem copied out, or with ``copy=False`` a VIEW of it (the reference's contract, Gi.cpp:3003-3006:
        the pointer stays valid, its contents are those of the last render, until the buffer is destroyed) -- or None when ``device_only``."""
        L = self.L
        rb = self.color_buffer(width, height)
        L.giCSetRenderBufferDeviceOnly(rb, int(device_only))
        binding = GiCAovBinding()
        binding.aovId = AOV_COLOR
        clear = np.asarray(settings.clear_color, np.float32)
        C.memmove(binding.clearValue, clear.ctypes.data, 16)
        binding.renderBuffer = rb
        p = GiCRenderParams()
        p.aovBindings = C.pointer(binding)
        p.aovBindingCount = 1
        p.camera = _camera(self.desc.camera)
        p.domeLight = self.dome
        p.renderSettings = _settings(settings)
        p.scene = self.handle
        r0, r1 = rows if rows is not None else (0, height)
        p.rowBegin, p.rowEnd, p.rowStride = r0, r1, row_stride
        if L.giCRender(C.byref(p)) != GI_C_OK:
            raise GiError("giCRender failed: " + L.giCGetLastError().decode())
        if device_only:
            return None
        mem = L.giCGetRenderBufferMem(rb)
        full = np.ctypeslib.as_array(C.cast(mem, C.POINTER(C.c_float)), shape=(height, width, 4))
        return full[r0:r1:row_stride].copy() if copy else full[r0:r1:row_stride]

    AOVS = {"normal": (1, FORMAT_FLOAT32_VEC4), "nee": (2, FORMAT_FLOAT32_VEC4), "barycentrics": (3, FORMAT_FLOAT32_VEC4),
            "texcoords": (4, FORMAT_FLOAT32_VEC4), "bounces": (5, FORMAT_FLOAT32_VEC4), "clockCycles": (6, FORMAT_FLOAT32_VEC4), "opacity": (7, FORMAT_FLOAT32_VEC4),
            "tangents": (8, FORMAT_FLOAT32_VEC4), "bitangents": (9, FORMAT_FLOAT32_VEC4), "thinWalled": (10, FORMAT_FLOAT32_VEC4),
            "objectId": (11, FORMAT_INT32), "depth": (12, FORMAT_FLOAT32), "faceId": (13, FORMAT_INT32), "instanceId": (14, FORMAT_INT32),
            "doubleSided": (15, FORMAT_FLOAT32_VEC4), "albedo": (16, FORMAT_FLOAT32_VEC4),
            # GI_C_AOV_EXT_MOMENTS: per pixel (S1, S2, n, 0) over the luminance of the accumulation's samples; the clear value is not used
            "moments": (AOV_EXT_MOMENTS, FORMAT_FLOAT32_VEC4)}

    def render_aovs(self, settings: RenderSettings, width: int, height: int, names, clear_values=None, with_color=True, rows=None, row_stride=1):
        """One giCRender call with the colour AOV (optional) plus the named non-colour AOVs bound (Gi.h:36-56, 161-166).
        Returns {name: array}; vec3 AOVs come back as [h, w, 4] (the shader writes .xyz only), ids / depth as [h, w]."""
        L = self.L
        r0, r1 = rows if rows is not None else (0, height)
        bindings = []
        bufs = {}
        if with_color:
            bufs["color"] = (self.color_buffer(width, height), FORMAT_FLOAT32_VEC4, np.asarray(settings.clear_color, np.float32).tobytes(), AOV_COLOR)
        for name in names:
            aid, fmt = self.AOVS[name]
            key = ("aov", name, width, height)
            if key not in self._buffers:
                self._buffers[key] = L.giCCreateRenderBuffer(width, height, fmt)
            cv = (clear_values or {}).get(name, 0)
            if fmt == FORMAT_INT32:
                raw = np.int32(cv).tobytes() + b"\0" * 12
            elif fmt == FORMAT_FLOAT32:
                raw = np.float32(cv).tobytes() + b"\0" * 12
            else:
                cv4 = (list(cv) + [0, 0, 0, 0])[:4] if hasattr(cv, "__len__") else [cv] * 4
                raw = np.asarray(cv4, np.float32).tobytes()
            bufs[name] = (self._buffers[key], fmt, raw, aid)
        arr = (GiCAovBinding * len(bufs))()
        for i, (name, (rb, fmt, raw, aid)) in enumerate(bufs.items()):
            arr[i].aovId = aid
            C.memmove(arr[i].clearValue, raw, 16)
            arr[i].renderBuffer = rb
        p = GiCRenderParams()
        p.aovBindings = C.cast(arr, C.POINTER(GiCAovBinding)); p.aovBindingCount = len(bufs)
        p.camera = _camera(self.desc.camera); p.domeLight = self.dome; p.renderSettings = _settings(settings); p.scene = self.handle
        p.rowBegin, p.rowEnd, p.rowStride = r0, r1, row_stride
        self._last_aovs = None
        if L.giCRender(C.byref(p)) != GI_C_OK:
            raise GiError("giCRender failed: " + L.giCGetLastError().decode())
        self._last_aovs = (width, height, {name: rb for name, (rb, fmt, raw, aid) in bufs.items()})
        out = {}
        for name, (rb, fmt, raw, aid) in bufs.items():
            mem = L.giCGetRenderBufferMem(rb)
            if fmt == FORMAT_FLOAT32_VEC4:
                a = np.ctypeslib.as_array(C.cast(mem, C.POINTER(C.c_float)), shape=(height, width, 4))
            elif fmt == FORMAT_FLOAT32:
                a = np.ctypeslib.as_array(C.cast(mem, C.POINTER(C.c_float)), shape=(height, width))
            else:
                a = np.ctypeslib.as_array(C.cast(mem, C.POINTER(C.c_int32)), shape=(height, width))
            out[name] = a[r0:r1:row_stride].copy()
        return out

    def aov_host_array(self, name: str, width: int, height: int):
        """The whole host copy of the buffer render_aovs keeps for `name` at this size, every row of it (render_aovs returns the rendered rows alone)."""
        rb = self._buffers[("aov", name, width, height)]
        fmt = self.AOVS[name][1]
        ctype, shape = (C.c_float, (height, width, 4)) if fmt == FORMAT_FLOAT32_VEC4 else ((C.c_float if fmt == FORMAT_FLOAT32 else C.c_int32), (height, width))
        return np.ctypeslib.as_array(C.cast(self.L.giCGetRenderBufferMem(rb), C.POINTER(ctype)), shape=shape).copy()

    def denoise_last(self, device_only=False, variance=False, **params):
        """giCDenoise on the buffers of the last render_aovs, which must have bound the colour, "normal" and "depth" (clear value = backgroundDepth, 1.0 by
        default); "albedo" is used when it was bound.  source defaults to GI_C_DENOISE_SOURCE_AUTO: the device copies where that render was a whole frame on
        the primary device.  Returns the filtered image float32 [h, w, 4] (None with ``device_only``); the output buffer is the scene's own, kept per size.
        ``variance=True``: giCDenoiseVariance with the "moments" buffer that render bound (the parameters then take sigmaVariance, varianceFloor, minSamples)."""
        if not getattr(self, "_last_aovs", None):
            raise GiError("denoise_last: no render_aovs call to take the buffers from")
        width, height, bufs = self._last_aovs
        for name in ("color", "normal", "depth") + (("moments",) if variance else ()):
            if name not in bufs:
                raise GiError(f"denoise_last: the last render_aovs did not bind {name!r}")
        L = self.L
        key = ("denoised", width, height)
        if key not in self._buffers:
            rb = L.giCCreateRenderBuffer(width, height, FORMAT_FLOAT32_VEC4)
            if not rb:
                raise GiError("giCCreateRenderBuffer failed: " + L.giCGetLastError().decode())
            self._buffers[key] = rb
        out_rb = self._buffers[key]
        L.giCSetRenderBufferDeviceOnly(out_rb, int(device_only))
        vp = denoise_variance_params(**params) if variance else None
        p = vp.base if variance else denoise_params(**params)
        p.color, p.normal, p.depth, p.albedo, p.output = bufs["color"], bufs["normal"], bufs["depth"], bufs.get("albedo"), out_rb
        if variance:
            vp.moments = bufs["moments"]
            if L.giCDenoiseVariance(C.byref(vp)) != GI_C_OK:
                raise GiError("giCDenoiseVariance failed: " + L.giCGetLastError().decode())
        elif L.giCDenoise(C.byref(p)) != GI_C_OK:
            raise GiError("giCDenoise failed: " + L.giCGetLastError().decode())
        if device_only:
            return None
        mem = L.giCGetRenderBufferMem(out_rb)
        return np.ctypeslib.as_array(C.cast(mem, C.POINTER(C.c_float)), shape=(height, width, 4)).copy()

    def device_pointer(self, width, height) -> int:
        return int(self.L.giCGetRenderBufferDeviceMem(self.color_buffer(width, height)))

    def stats(self) -> dict:
        s = GiCRenderStats()
        if self.L.giCGetRenderStats(self.handle, C.byref(s)) != GI_C_OK:
            raise GiError("giCGetRenderStats failed")
        return {name: getattr(s, name) for name, _ in GiCRenderStats._fields_}

    def lookahead_stats(self) -> dict:
        """giCGetLookaheadStats: the sample look-ahead window as the last render left it, and the totals since the scene was created."""
        s = GiCLookaheadStats()
        if self.L.giCGetLookaheadStats(self.handle, C.byref(s)) != GI_C_OK:
            raise GiError("giCGetLookaheadStats failed")
        return {name: getattr(s, name) for name, _ in GiCLookaheadStats._fields_ if name != "reserved"}

    def trace_rays(self, origins, dirs, t_min=0.0, t_max=3.0e38):
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = len(o)
        tuv = np.zeros((n, 3), np.float32)
        ip = np.zeros((n, 2), np.int32)
        rc = self.L.giCTraceRays(self.handle, n, o.ctypes.data_as(_FP), d.ctypes.data_as(_FP), t_min, t_max,
                                 tuv.ctypes.data_as(_FP), ip.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc < 0:
            raise GiError("giCTraceRays failed: " + self.L.giCGetLastError().decode())
        return tuv, ip

    def validate_bvh(self, device: int = 0) -> dict:
        """giCDebugValidateSceneBvh: the tree resident on `device` (0 = primary) of a scene rendered at least once, downloaded and checked.
        Returns {"violations", "nodes", "depth", "device_built", "digest"}."""
        nodes, depth, built, digest = C.c_uint32(0), C.c_uint32(0), C.c_int32(0), C.c_uint64(0)
        v = self.L.giCDebugValidateSceneBvh(self.handle, device, C.byref(nodes), C.byref(depth), C.byref(built), C.byref(digest))
        if v < 0:
            raise GiError("giCDebugValidateSceneBvh failed: " + self.L.giCGetLastError().decode())
        return {"violations": v, "nodes": nodes.value, "depth": depth.value, "device_built": bool(built.value), "digest": digest.value}

    def close(self):
        if self.handle:
            L = self.L
            for rb in self._buffers.values():
                L.giCDestroyRenderBuffer(rb)
            self._buffers = {}
            destroy = {"sphere": L.giCDestroySphereLight, "distant": L.giCDestroyDistantLight, "rect": L.giCDestroyRectLight,
                       "disk": L.giCDestroyDiskLight}
            for kind, h in self.lights:
                destroy[kind](self.handle, h)
            for h in self.meshes:
                L.giCDestroyMesh(h)
            for h in self.materials:
                if h:
                    L.giCDestroyMaterial(h)
            if self.dome:
                L.giCDestroyDomeLight(self.dome)
            for h in self.textures:
                L.giCDestroyTexture(h)
            self.lights, self.meshes, self.materials, self.textures, self.dome = [], [], [], [], None
            self.L.giCDestroyScene(self.handle)
            self.handle = None


def shade_class(material) -> int:
    """giCDebugShadeClass: the k_shade variant (shade class) of an untextured material; host only."""
    md = GiCMaterialDesc(material.klass, 0, (C.c_float * P_COUNT)(*np.asarray(material.params, np.float32)))
    return int(load_library().giCDebugShadeClass(C.byref(md)))


UPS_NOCOAT = 1  # gi_types.h: the trait of a scene's UsdPreviewSurface materials (Scene.ups_plain)


def ups_traits(records, derive: bool = True) -> int:
    """giCDebugUpsTraits: the traits of a material table alone; host only.  `records`: (klass, flags, params[64]) triples -- with `derive` the parameters are a
    material description's, without it a derived record's, word for word (so float32 arrays keep the bits they were given)."""
    descs = (GiCMaterialDesc * max(len(records), 1))()
    for d, (klass, flags, params) in zip(descs, records):
        d.klass, d.flags = klass, flags
        C.memmove(d.p, np.ascontiguousarray(params, np.float32).ctypes.data, 4 * P_COUNT)
    out = C.c_uint32(0)
    if load_library().giCDebugUpsTraits(descs, len(records), 1 if derive else 0, C.byref(out)) != GI_C_OK:
        raise GiError("giCDebugUpsTraits failed")
    return int(out.value)


def bsdf_debug(material, items, device: int = 0):
    """Device-side closed-form BSDF sample/evaluate; items float32 [n,22] -> float32 [n,15] (see include/gi_c.h)."""
    L = initialize(device)
    md = GiCMaterialDesc(material.klass, 0, (C.c_float * P_COUNT)(*np.asarray(material.params, np.float32)))
    a = np.ascontiguousarray(items, np.float32).reshape(-1, 22)
    out = np.zeros((len(a), 15), np.float32)
    if L.giCDebugEvalBsdf(C.byref(md), len(a), a.ctypes.data_as(_FP), out.ctypes.data_as(_FP)) != GI_C_OK:
        raise GiError("giCDebugEvalBsdf failed: " + L.giCGetLastError().decode())
    return out
