// Host-side scene model: reads Tungsten's JSON scene format and prepares the render-time
// quantities the reference computes in its prepareForRender() methods.  No intersection
// or shading code lives here -- that is all on the GPU (csrc/hip) -- these classes only
// hold parameters and mirror the reference's loading semantics:
//   Scene::load/fromJson        src/core/io/Scene.cpp:236-253,378-391
//   Primitive::fromJson         src/core/primitives/Primitive.cpp:22-32
//   Bsdf::fromJson              src/core/bsdfs/Bsdf.cpp:19-25
//   Camera::fromJson            src/core/cameras/Camera.cpp:44-68
//   RendererSettings::fromJson  src/core/renderer/RendererSettings.hpp:49-76
#ifndef TGAMD_SCENE_HPP_
#define TGAMD_SCENE_HPP_

#include "Json.hpp"
#include "Math.hpp"

#include <memory>
#include <string>
#include <vector>

namespace tungsten_amd {

// ---- textures (src/core/textures) ---------------------------------------------------
struct Texture
{
    enum Type { Constant = 0, Checker = 1, Bitmap = 2, Disk = 3, Blade = 4 };   // (an `ies` texture is a Bitmap whose texels bakeIes() wrote)
    Type type = Constant;
    Vec3f value = Vec3f(1.0f);                 // ConstantTexture; DiskTexture / BladeTexture: _value
    // BladeTexture (textures/BladeTexture.cpp:14-31): _numBlades, _angle and what init() derives from them
    int blades = 6;
    float bladeOffset = 0.5f*PI/6, bladeAngle = 0.0f, bladeArea = 0.0f;
    float bladeEdge[2] = {0.0f, 0.0f}, bladeNormal[2] = {0.0f, 0.0f};
    void initBlade();
    // IesTexture (textures/IesTexture.cpp): the profile baked into 2 resolution x resolution scalar texels
    bool ies = false;
    int iesResolution = 256;
    void bakeIes(const std::string &file);     // IesTexture::loadResources + BitmapTexture::init
    Vec3f onColor = Vec3f(0.8f), offColor = Vec3f(0.2f); // CheckerTexture.cpp:11-30
    int resU = 20, resV = 20;
    // BitmapTexture: float texels (.hdr), or 8-bit ones (.png) converted once to the floats the reference's lookups produce
    std::string path;
    int w = 0, h = 0;
    bool rgb = true, linear = true, clamp = false, valid = false;
    bool gammaCorrect = true;                  // LDR RGB textures only (io/ImageIO.cpp:515-518)
    bool autoAlpha = false;                    // scalar request REQUEST_AUTO instead of REQUEST_AVERAGE (Scene::fetchTexture)
    float scale = 1.0f;
    std::vector<float> texels;                 // rgb ? 3*w*h : w*h
    Vec3f texMin, texMax, texAvg;
    // Distribution2D (sampling/Distribution2D.hpp), built by makeSamplable(MAP_SPHERICAL)
    bool samplable = false;
    std::vector<float> marginalPdf, marginalCdf, pdf, cdf;

    bool isConstant() const { return type == Constant; }
    Vec3f average() const;
    Vec3f maximum() const;
    void scaleValues(float f);
    void makeSamplable(bool spherical);        // BitmapTexture::makeSamplable(MAP_SPHERICAL / MAP_UNIFORM), BitmapTexture.cpp:400-431
    void makeSamplableSpherical() { makeSamplable(true); }
    void loadBitmap(const std::string &file);  // BitmapTexture::loadResources + init
    void finishBitmap();                       // BitmapTexture::init's statistics over `texels` (w, h, rgb set)
};

// ---- BSDFs (src/core/bsdfs) ------------------------------------------------------------
struct Bsdf
{
    enum Type { Lambert = 0, Null = 1, RoughConductor = 2, SmoothCoat = 3, Dielectric = 4, RoughDielectric = 5,
                Mirror = 6, Conductor = 7, Plastic = 8, RoughPlastic = 9, Mixed = 10, Transparency = 11,
                Forward = 12, Error = 13, DiffuseTransmission = 14, Phong = 15, ThinSheet = 16, OrenNayar = 17, RoughCoat = 18,
                LambertianFiber = 19, RoughWire = 20 };
    std::string name;
    Type type = Lambert;
    unsigned lobes = 0;
    std::shared_ptr<Texture> albedo, roughness, tex1;
    std::shared_ptr<Texture> bump;              // a non-constant bump map (Bsdf::_bump), else null
    std::shared_ptr<Bsdf> sub0, sub1;
    int distribution = 2;                       // 0 beckmann, 1 phong, 2 ggx
    float ior = 1.5f, thickness = 1.0f;
    bool enableRefraction = true;
    Vec3f eta = Vec3f(0.200438f, 0.924033f, 1.10221f), k = Vec3f(3.91295f, 2.45285f, 2.14219f);
    Vec3f sigmaA = Vec3f(0.0f), scaledSigmaA = Vec3f(0.0f);
    float avgTransmittance = 1.0f, diffuseFresnel = 0.0f;
    float exponent = 64.0f, diffuseRatio = 0.2f;   // PhongBsdf (PhongBsdf.hpp: defaults of its constructor)
    float wireRoughness = 0.1f;                 // RoughWireBcsdf::_roughness, a plain float (RoughWireBcsdf.cpp:17-25, 100); prepareForRender leaves _v in `thickness`
    bool prepared = false;

    bool unnamed() const { return name.empty(); }
    void prepareForRender();
};

// ---- participating media (src/core/media, phasefunctions, transmittances) ----------------
struct Medium   // media/HomogeneousMedium.{hpp,cpp} + Medium.cpp + transmittances/*.cpp
{
    std::string name;
    Vec3f materialSigmaA = Vec3f(0.0f), materialSigmaS = Vec3f(0.0f);
    float density = 1.0f;
    int maxBounce = 1024;
    int mediumType = 0;         // TGHIP_MEDIUM_*: 0 homogeneous, 1 exponential (media/ExponentialMedium.cpp), 2 atmosphere (media/AtmosphericMedium.cpp)
    float radius = 1.0f;        // AtmosphericMedium.cpp:14-23: _radius, _center, the pivot primitive's name (its origin replaces _center, :68-77)
    Vec3f center = Vec3f(0.0f);
    std::string pivot;
    float effectiveFalloffScale = 1.0f;   // _falloffScale/_radius (:79)
    float falloffScale = 1.0f;  // ExponentialMedium.cpp:12-19
    Vec3f unitPoint = Vec3f(0.0f), falloffDirection = Vec3f(0.0f, 1.0f, 0.0f), unitFalloffDirection = Vec3f(0.0f, 1.0f, 0.0f);
    int phaseType = 0;          // 0 isotropic, 1 henyey_greenstein, 2 rayleigh
    float phaseG = 0.0f;
    int transType = 0;          // TGHIP_TRANS_*: exponential, linear, quadratic, double_exponential, pulse, erlang
    float transP[3] = {0.0f, 0.0f, 0.0f};
    // interpolated (transType 8): transP[0] = ratio, operands _trA / _trB (InterpolatedTransmittance.cpp:15-29)
    int subType[2] = {1, 5};
    float subP[2][3] = {{1.0f, 0.0f, 0.0f}, {5.0f, 0.0f, 0.0f}};
    // prepareForRender (HomogeneousMedium.cpp:43-49)
    Vec3f sigmaA, sigmaS, sigmaT;
    bool absorptionOnly = false;
    void prepareForRender();
};

// ---- primitives (src/core/primitives) ----------------------------------------------------
struct MeshVertex { float pos[3], normal[3], uv[2]; };          // Vertex.hpp:10-13 (32 B, .wo3 layout)
struct MeshTriangle { uint32_t v0, v1, v2; int32_t material; };  // Triangle.hpp:14-28 (16 B)

// The box of an instance's geometry: the master's vertices (3 floats every strideFloats) rotated by q, translated by pos, padded for the rounding
// of the device's own world -> master transform, never larger than the reference's box of the instance (Primitive::tightenInstanceBounds;
// tgh_instance_tight_bounds for the reference-side flattener)
Box3f tightInstanceBox(const float *vertexPositions, size_t strideFloats, size_t numVertices, const QuaternionF &q, const Vec3f &pos, const Box3f &refBox);

struct Primitive
{
    // (the values of the first ten are TGHIP_OBJ_*; a Skydome is flattened to TGHIP_OBJ_INFINITE_SPHERE | TGHIP_OBJF_SKYDOME)
    enum Type { Mesh = 0, Quad = 1, Cube = 2, Sphere = 3, InfiniteSphere = 4, Instances = 5, Disk = 6, InfiniteSphereCap = 7, Point = 8, Cylinder = 9, Skydome = 10 };
    std::string name;
    Type type = Quad;
    Mat4f transform;
    std::shared_ptr<Texture> emission, power;
    std::vector<std::shared_ptr<Bsdf>> bsdfs;
    std::shared_ptr<Medium> intMedium, extMedium;   // Primitive.cpp:30-31
    // mesh
    std::string file;
    bool smooth = false, backfaceCulling = false, recomputeNormals = false;
    std::vector<MeshVertex> verts, tfVerts;
    std::vector<MeshTriangle> tris;
    // infinite sphere
    bool doSample = true;
    // skydome (primitives/Skydome.cpp:18-26, 68-77): the star's temperature in kelvin, the atmosphere's turbidity, the star's brightness
    // relative to the sun ("gamma_scale" is read and never used by the reference: fillImage is called with 1, :298)
    float skyTemperature = 5777.0f, skyTurbidity = 3.0f, skyIntensity = 2.0f;
    bool capped = true;         // cylinder (primitives/Cylinder.hpp)
    // disk (primitives/Disk.hpp): emission confined to a cone around the normal
    float coneAngle = 90.0f;
    // infinite sphere cap (primitives/InfiniteSphereCap.hpp): emission from directions within cap_angle of the transform's up axis
    float capAngleDeg = 10.0f;
    // "skydome": the name of the primitive whose transform gives the cap its direction (InfiniteSphereCap.cpp:233-250); Scene::fromJson resolves it
    // once every primitive exists, as _scene->findPrimitive would at prepareForRender
    std::string domeName;
    bool pivoted = false;
    Mat4f pivotTransform;
    // instances (primitives/Instance.hpp:13-31): rigid placements (position + rotation) of master primitives
    std::vector<std::shared_ptr<Primitive>> masters;
    std::string instanceFile;
    std::vector<Vec3f> instancePos;
    std::vector<QuaternionF> instanceRot;
    std::vector<uint8_t> instanceId;
    std::vector<Box3f> instanceBounds;      // prepareForRender: tight world-space box of every instance (tightenInstanceBounds)
    std::vector<Box3f> instanceRefBounds;   // prepareForRender: world-space box of every instance as the reference boxes it (Instance.cpp:409-421:
                                            // the master box's eight rotated corners): what its own BVH over the instances is built from and
                                            // tested against (RefInstanceBvh.hpp)

    // prepared (prepareForRender of the respective reference class)
    Vec3f base, edge0, edge1, normal; float invUvSq[2] = {0, 0};  // Quad.cpp:298-316
    Vec3f pos, scale; Mat4f rot, invRot; Vec3f faceCdf;            // Cube.cpp:353-370 / Sphere / InfiniteSphere.cpp:280-286
    float area = 0.0f, invArea = 0.0f;
    Box3f bounds;

    bool isInfinite() const { return type == InfiniteSphere || type == InfiniteSphereCap || type == Skydome; }
    bool isDirac() const { return type == Point || (type == Mesh && (verts.empty() || tris.empty())); }   // Point.cpp:156-159, TriangleMesh.cpp
    bool isEmissive() const;       // Primitive.hpp:111-115
    bool isSamplable() const { return isInfinite() ? doSample : type != Instances; }   // Instance.cpp:357-360
    float powerToRadianceFactor() const;
    void loadResources(const std::string &sceneDir);
    void prepareForRender();
    void tightenInstanceBounds();
};

// ---- camera ------------------------------------------------------------------------------
struct Camera
{
    std::string tonemap = "gamma";
    std::string filterName = "tent";
    unsigned resX = 1000, resY = 563;
    Mat4f transform;
    Vec3f pos, lookAt, up;
    float fovDeg = 60.0f;
    // cameras/ThinlensCamera.cpp:16-27 (type "thinlens"; the aperture is the default DiskTexture)
    bool thinlens = false;
    bool equirectangular = false;                   // cameras/EquirectangularCamera.cpp (type "equirectangular")
    int cubemapMode = -1;                           // cameras/CubemapCamera.cpp (type "cubemap"): 0 horizontal_cross, 1 vertical_cross, 2 row, 3 column; -1 = not a cubemap camera
    float focusDist = 1.0f, apertureSize = 0.001f, catEye = 0.0f;
    // "aperture": {"type": "blade", "blades": n, "angle": a} (textures/BladeTexture.cpp:14-41); 0 blades = the disk
    int blades = 0;
    // "aperture": a bitmap (a file name or {"type": "bitmap", ...}; scalar request REQUEST_AVERAGE, ThinlensCamera.cpp:62-63): the lens
    // point is drawn from the image (BitmapTexture::sample with the MAP_UNIFORM distribution); an `ies` aperture is such a bitmap (its bake);
    // a constant or a checker: the lens point is ConstantTexture::sample's / CheckerTexture::sample's (non-bitmaps ignore the scalar request)
    std::shared_ptr<Texture> apertureTex;
    float bladeAngle = 0.0f, bladeStep = 0.0f;
    float bladeEdge[2] = {0.0f, 0.0f};
    Mat4f invTransform;
    std::shared_ptr<Medium> medium;                 // Camera.cpp:49-50
    // precompute()
    float ratio = 0, pixelSizeX = 0, planeDist = 0;
    // ReconstructionFilter::precompute (cameras/ReconstructionFilter.cpp:34-58)
    int filterType = 2; float filterWidth = 1.0f, filterBinSize = 0; float filterCdf[32];

    Camera();
    void fromJson(const JsonValue &v, const class Scene &scene);
    void precompute();
};

struct OutputBufferSettings   // cameras/OutputBufferSettings.{hpp,cpp}
{
    int type = 0;                            // TGHIP_AUX_*: color, depth, normal, albedo, visibility
    std::string ldrOutputFile, hdrOutputFile;
    bool twoBufferVariance = false, sampleVariance = false;
};

struct RendererSettings   // renderer/RendererSettings.hpp:15-107
{
    std::vector<OutputBufferSettings> outputs;   // "output_buffers" (RendererSettings.hpp:70-75)
    std::string outputFile = "TungstenRender.png", hdrOutputFile, resumeRenderFile = "TungstenRenderState.dat";
    bool overwriteOutputFiles = true, useAdaptiveSampling = true, enableResumeRender = false, useSobol = true, useSceneBvh = true;
    unsigned spp = 32, sppStep = 16;
    void fromJson(const JsonValue &v);
};

struct IntegratorSettings // TraceSettings.hpp:15-39 + PathTracerSettings.hpp:17-43
{
    std::string type = "path_tracer";
    int minBounces = 0, maxBounces = 64;
    bool enableConsistencyChecks = false, enableTwoSidedShading = true;
    bool enableLightSampling = true, enableVolumeLightSampling = true, lowOrderScattering = true, includeSurfaces = true;
    int devices = 1;             // path_tracer_hip extension: GPUs used by one integrator
    bool shareDevices = false;   // path_tracer_hip extension ("share_devices"): `devices` contexts even on fewer GPUs, dealt round-robin
                                 // (several tile shards, each driven by its own host thread, on one device: how the multi-device path
                                 // is exercised on a single-GPU box)
    void fromJson(const JsonValue &v);
};

class Scene
{
    friend struct Camera;                      // (a thin-lens camera's bitmap aperture goes through fetchTexture)
    std::string _srcDir;
    mutable std::vector<std::pair<std::string, std::shared_ptr<Texture>>> _textureCache;
    mutable std::vector<std::shared_ptr<Texture>> _iesTextures;   // (TextureCache serves bitmaps only: every `ies` texture is baked on its own)

    // autoAlpha: TexelConversion::REQUEST_AUTO (TransparencyBsdf's "alpha"): the alpha channel where the decoder reports one -- for a .png
    // always (io/ImageIO.cpp:386-407 decodes to RGBA and reports 4 channels) --, else the average
    std::shared_ptr<Texture> fetchTexture(const JsonValue &v, bool rgb, bool autoAlpha = false) const;  // Scene.cpp:127-151
    std::shared_ptr<Bsdf> fetchBsdf(const JsonValue &v) const;                  // Scene.cpp:82-93
    std::shared_ptr<Bsdf> instantiateBsdf(const JsonValue &v) const;
    std::shared_ptr<Primitive> instantiatePrimitive(const JsonValue &v) const;
    std::shared_ptr<Primitive> fetchPrimitive(const JsonValue &v) const;          // Scene.cpp:82-93
    std::shared_ptr<Medium> instantiateMedium(const JsonValue &v) const;

public:
    std::shared_ptr<Medium> fetchMedium(const JsonValue &v) const;               // Scene.cpp:105-108
    std::vector<std::shared_ptr<Medium>> media;
    std::vector<std::shared_ptr<Bsdf>> bsdfs;
    std::vector<std::shared_ptr<Primitive>> primitives;
    Camera camera;
    IntegratorSettings integrator;
    RendererSettings renderer;

    static std::unique_ptr<Scene> load(const std::string &jsonPath);   // Scene::load + loadResources
    void fromJson(const JsonValue &root);
    void loadResources();
    const std::string &srcDir() const { return _srcDir; }
};

} // namespace tungsten_amd

#endif
