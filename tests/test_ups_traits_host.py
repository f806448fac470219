"""The traits of a scene's UsdPreviewSurface materials (gi_build.cpp upsTraitsOf / deriveSceneClasses), held on material tables alone through giCDebugUpsTraits,
without a GPU: NOCOAT needs the coat's word to be that of +0.0f in every class-1 record, whatever its F0; a textured class-1 record does not have it; records
of other classes do not count, and a table without a class-1 record has no traits."""
import numpy as np

from gatling_amd import capi
from gatling_amd.scene import MAT_DIFFUSE, MAT_OPEN_PBR, MAT_USD_PREVIEW_SURFACE, P_CLEARCOAT, MaterialDesc

NOCOAT = capi.UPS_NOCOAT
MP_F0, MP_COAT = 35, 39  # gi_types.h
TEXTURED = 1 << 31       # MAT_FLAG_TEXTURED


def _ups(**kw):
    return (MAT_USD_PREVIEW_SURFACE, 0, MaterialDesc.usd_preview_surface(**kw).params)


def test_descriptions():
    plain = _ups(diffuseColor=(1, 0, 0))
    assert capi.ups_traits([plain]) == NOCOAT
    assert capi.ups_traits([plain, _ups(roughness=0.0), _ups(ior=1.0), _ups(ior=2.5, diffuseColor=(0, 1, 0))]) == NOCOAT
    assert capi.ups_traits([plain, _ups(clearcoat=0.5)]) == 0
    assert capi.ups_traits([plain, _ups(clearcoat=1e-30)]) == 0
    assert capi.ups_traits([plain, _ups(metallic=1.0, diffuseColor=(1, 0.5, 0.25))]) == NOCOAT
    assert capi.ups_traits([plain, _ups(metallic=1.0, diffuseColor=(0.5, 0.5, 0.5))]) == NOCOAT
    assert capi.ups_traits([plain, _ups(useSpecularWorkflow=1, specularColor=(0.3, 0.3, 0.3))]) == NOCOAT
    assert capi.ups_traits([plain, _ups(useSpecularWorkflow=1, specularColor=(0.3, 0.2, 0.1))]) == NOCOAT
    assert capi.ups_traits([_ups(clearcoat=0.5, metallic=0.5, diffuseColor=(1, 0, 0)), plain]) == 0


def test_negative_zero_and_nan_coats_do_not_qualify():
    minus = _ups(clearcoat=-0.0)
    assert minus[2][P_CLEARCOAT] == 0.0 and np.signbit(minus[2][P_CLEARCOAT])
    assert capi.ups_traits([minus]) == 0
    assert capi.ups_traits([_ups(clearcoat=float("nan"))]) == 0
    # ... and on derived records, word for word
    rec = np.zeros(64, np.float32); rec[MP_F0:MP_F0 + 3] = 0.04
    assert capi.ups_traits([(1, 0, rec)], derive=False) == NOCOAT
    for word in (0x80000000, 0x7fc00000, 0xffc00000, 0x00000001):
        r = rec.copy(); r.view(np.uint32)[MP_COAT] = word
        assert capi.ups_traits([(1, 0, r)], derive=False) == 0, hex(word)


def test_f0_does_not_matter():
    rec = np.zeros(64, np.float32); rec[MP_F0:MP_F0 + 3] = (0.9, 0.04, 0.5)
    assert capi.ups_traits([(1, 0, rec)], derive=False) == NOCOAT
    r = rec.copy(); r.view(np.uint32)[MP_F0:MP_F0 + 3] = 0x7fc00000
    assert capi.ups_traits([(1, 0, r)], derive=False) == NOCOAT


def test_textured_records_and_other_classes():
    plain = _ups()
    assert capi.ups_traits([plain, (MAT_USD_PREVIEW_SURFACE, TEXTURED, plain[2])]) == 0  # ups_params recomputes F0 and alpha from texture values
    assert capi.ups_traits([]) == 0
    assert capi.ups_traits([(MAT_DIFFUSE, 0, plain[2])]) == 0
    pbr = MaterialDesc.open_pbr(coat_weight=1.0)
    assert capi.ups_traits([(MAT_OPEN_PBR, 0, pbr.params)]) == 0
    assert capi.ups_traits([plain, (MAT_DIFFUSE, 0, _ups(clearcoat=0.5)[2]), (MAT_OPEN_PBR, 0, pbr.params)]) == NOCOAT  # only class-1 records count
