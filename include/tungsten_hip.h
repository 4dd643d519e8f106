/*
 * tungsten_hip.h -- C-ABI boundary of the MI355X-native `path_tracer_hip` integrator.
 *
 * This is the thin extern "C" shim the north star asks for: plain pointers and sizes,
 * no C++/torch types.  It is what a Tungsten maintainer would bind from the reference's
 * C++11 host.  Each entry point names the reference interface it
 * replaces (paths relative to the reference tree, src/core/...):
 *
 *   tghip_upload_scene      <- TraceableScene::TraceableScene (renderer/TraceableScene.hpp:57-137):
 *                              the Embree top-level + per-mesh scenes (primitives/TriangleMesh.cpp:524-572)
 *                              become one flattened BVH2 + SoA record stream in HBM.
 *   tghip_render_pass/_wait <- PathTraceIntegrator::startRender / waitForCompletion
 *                              (integrators/path_tracer/PathTraceIntegrator.cpp:220-244) and, inside them,
 *                              renderTile (:136-156) -> PathTracer::traceSample (PathTracer.cpp:14-149).
 *   tghip_abort             <- PathTraceIntegrator::abortRender (PathTraceIntegrator.cpp:246-256).
 *   tghip_download_framebuffer <- OutputBuffer<Vec3f>::addSample / operator[] (cameras/OutputBuffer.hpp:104-144).
 *   tghip_trace_rays        <- TraceableScene::intersect (renderer/TraceableScene.hpp:170-192), batched.
 *   tghip_query_rays        <- TraceableScene::intersect and ::occluded (renderer/TraceableScene.hpp:170-223), batched, on host or device memory.
 *   tghip_query_surface     <- TraceableScene::intersect + Primitive::intersectionInfo (renderer/TraceableScene.hpp:170-192), the albedo and emission
 *                              of PathTracer.cpp:83-88 and TraceableScene::intersectInfinites (:194-209) for a miss, batched, on host or device memory.
 *   tghip_query_transmittance <- TraceBase::generalizedShadowRay (integrators/TraceBase.cpp:62-133), batched, on host or device memory.
 *   tghip_query_direct      <- TraceBase::estimateDirect / volumeEstimateDirect (integrators/TraceBase.cpp:470-494), batched, on host or device memory.
 *   tghip_query_vertex      <- one turn of PathTracer::traceSample's loop (PathTracer.cpp:50-131) on paths whose state the caller holds, batched, on
 *                              host or device memory.
 *   tghip_reduce_framebuffers <- the merge of per-machine partial renders the reference does offline on the host
 *                              (src/hdrmanip/hdrmanip.cpp:69-112: load N HDR images, add, divide); here the tile shards of
 *                              one frame, summed on the device side by RCCL over xGMI.
 *   tghip_comm_unique_id / tghip_comm_init_rank / tghip_reduce_framebuffer_rank <- the same merge with one PROCESS per GPU (hdrmanip.cpp:69-112
 *                              again: there the partial renders come from separate `tungsten` processes).
 *   tghip_get_counters      <- (no reference analogue; feeds the roofline model).
 *   tghip_get_walk_stats    <- (no reference analogue; lane utilisation of the walks).
 *   tghip_debug_libm        <- std::sin / cos / log / exp / acos / atan2 / pow / cbrt on floats as the reference's path calls them (glibc's sinf ... cbrtf):
 *                              the device's restatements evaluated on the device, for the parity tests.
 *   tghip_debug_bsdf / tghip_debug_bsdf_info <- Bsdf::eval / pdf / sample (bsdfs/Bsdf.hpp:71-97) of single scatter events: the shading kernels'
 *                              BSDF code on caller-supplied cases, per shading family, for the parity tests.
 *   tghip_debug_light / tghip_debug_light_info <- TraceBase::chooseLight (integrators/TraceBase.cpp:416-459) and Primitive::sampleDirect / approximateRadiance /
 *                              intersect + intersectionInfo / evalDirect / directPdf of single calls: the shading kernels' light code, the same way.
 *   tghip_debug_medium      <- Medium::sampleDistance / transmittance (media/Medium.hpp:63-67) and PhaseFunction::eval / sample of single calls: the
 *                              shading and shadow kernels' medium code, the same way.
 *
 * Ownership: the caller owns every host array (borrowed for the duration of the call; the
 * shim copies with hipMemcpyAsync); the shim owns device memory behind the opaque handle.
 * All functions return 0 on success and a negative TGHIP_E_* code on failure (message via
 * tghip_last_error); nothing throws across the boundary.  One handle per device; calls on
 * one handle must be serialised by the caller; different handles may be driven from
 * different host threads.
 *
 * The flattened scene structs below are also the input of the CPU oracle (oracle/oracle.c),
 * so that the checker and the HIP path consume bit-identical inputs.
 */
#ifndef TUNGSTEN_HIP_H_
#define TUNGSTEN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGHIP_ABI_VERSION 10

/* ---- error codes ------------------------------------------------------------------ */
enum {
    TGHIP_OK            =  0,
    TGHIP_E_INVALID     = -1,  /* bad argument / inconsistent description */
    TGHIP_E_NODEVICE    = -2,  /* no HIP device / hipSetDevice failed     */
    TGHIP_E_HIP         = -3,  /* a HIP runtime call failed               */
    TGHIP_E_NOSCENE     = -4,  /* render/trace before upload              */
    TGHIP_E_ABORTED     = -5,  /* pass was aborted via tghip_abort        */
    TGHIP_E_UNSUPPORTED = -6   /* feature outside the hot-path scope      */
};

/* ---- flattened geometry -------------------------------------------------------------
 * One BVH2 over all finite primitives in world space (the reference bakes transforms into
 * _tfVerts, TriangleMesh.cpp:542-552).  64-byte nodes; a child reference is either an
 * internal node index (>= 0) or a leaf (bit 31 set): count = (ref >> 27) & 15, first record
 * = ref & 0x07FFFFFF.  Leaves are contiguous runs of 48-byte primitive records. */
/* a node of the reference's own BVH over the instances of an `instances` primitive as the host's restatement of its builder
 * produces it (bvh/BinaryBvh.hpp: TinyBvhNode): box = x: lmin rmin lmax rmax, then y, then z; count = 0: inner node, children
 * left and left + 1; else a leaf of `count` (1 or 2) instances at slots [left, left + count) of BinaryBvh::_primIndices.
 * Host-side only: the scene description carries these trees as TgHipBvhNode entries (see the instance-set record). */
typedef struct TgHipInstNode {
    float box[12];
    uint32_t left, count;
    uint32_t pad[2];
} TgHipInstNode;              /* 64 B */

typedef struct TgHipBvhNode {
    float   lo0[3], hi0[3];   /* child 0 bounds */
    float   lo1[3], hi1[3];   /* child 1 bounds */
    int32_t child0, child1;
    uint32_t pad[2];
} TgHipBvhNode;               /* 64 B */

#define TGHIP_LEAF_FLAG        0x80000000u
#define TGHIP_LEAF_COUNT(ref)  (((uint32_t)(ref) >> 27) & 15u)
#define TGHIP_LEAF_FIRST(ref)  ((uint32_t)(ref) & 0x07FFFFFFu)
#define TGHIP_MAKE_LEAF(first, count) (int32_t)(TGHIP_LEAF_FLAG | ((uint32_t)(count) << 27) | (uint32_t)(first))
#define TGHIP_MAX_LEAF         15
#define TGHIP_MAX_TREE_DEPTH   48   /* the builder's bound for ONE tree */
#define TGHIP_MAX_BVH_DEPTH    96   /* builder guarantees depth <= this (device stack size; single-level trees stay below 48, the
                                       three-level walk of scenes with instances adds the levels of its trees) */
/* Scenes with at most this many primitive records are intersected as a flat list in record order (every ray
 * tests every record; the wave walks the list uniformly, so record data comes through the scalar cache) instead of
 * through the BVH -- the analogue of the reference's top-level Embree scene over a handful of user-geometry
 * primitives (TraceableScene.hpp:112-134).  The oracle follows the same rule so that visit counts agree.
 * Flat lists with TgHipSceneDesc::top_nodes (scenes whose records are all quads, cubes, spheres, disks or cylinders): the closest hit is the one the reference's
 * Embree walk returns where faces coincide -- see TgHipTopNode below. */
#define TGHIP_FLAT_MAX_RECS    16

/* ---- the reference's top-level tree ----------------------------------------------------------------------------------------------
 * TraceableScene commits ONE Embree user geometry whose items are the scene's finite primitives (renderer/TraceableScene.hpp:112-134) and
 * Embree builds a BVH4 with one item per leaf over their bounds().  Where faces coincide -- a block standing ON the floor quad, a light lying
 * IN the ceiling, a ray into the seam of two walls -- the ORDER in which a ray visits that tree decides which primitive it hits
 * (kernels/bvh/bvh_intersector1.cpp:60-125, bvh_traverser1.h:41-104):
 *   - a child counts only if the ray passes its box by the node's slab test (rdir = rcp(dir) by RCPPS + one Newton step, planes
 *     (bound - org)*rdir, max / min and the comparison on the bit patterns as signed integers), under the hit distance found SO FAR;
 *   - of the children hit the nearest box entry is descended into first, the others wait on a stack sorted by entry (one hit child: go; two:
 *     the first only `if (d0 < d1)`; three / four: Embree's sorting networks, stack_item.h:44-60);
 *   - a child popped behind the hit found so far is skipped -- by its BOX's entry distance, which can lie an ulp behind the distance the
 *     primitive's own intersect() reports; a quad accepts t <= farT, a cube or sphere t < farT.
 * The tree is therefore part of the path's arithmetic.  csrc/host/EmbreeTopTree.cpp restates Embree 2.11's builder for it (binned SAH, four
 * children, leaf size one) node for node; tgh_top_tree_build (tungsten_host.h) produces it, tests/test_top_tree.py holds it to trees read out of
 * the reference's own Embree.  Scenes that carry it: flat lists of quads, cubes, spheres, disks and cylinders (one item per object that has a record, in
 * object order); every other scene passes NULL / 0 and is walked as before (a triangle mesh lives in ONE tree with the other records there).
 * Node 0 is the root, nodes in preorder.  child[i] >= 0: a node; < 0: the record ~child[i]; TGHIP_TOP_EMPTY: unused slot (its box is
 * lower = +inf, upper = -inf, as Embree clears it). */
#define TGHIP_TOP_EMPTY  0x7FFFFFFF
#define TGHIP_TOP_MAX_DEPTH 7       /* levels of nodes; Embree's tree over <= TGHIP_FLAT_MAX_RECS items has at most 5 (a node has four children or leaves only) */
typedef struct TgHipTopNode {
    float   lower[4][3];
    float   upper[4][3];
    int32_t child[4];
} TgHipTopNode;            /* 112 bytes */

/* ---- 8-wide BVH with quantised child boxes ------------------------------------------------------------------------
 * What the traversal kernels of single-level scenes walk (the BVH2 above stays the structure of the two-level
 * instance walk and of the transparency / media shadow walks).  It is the BVH2 collapsed: every wide node stands for a
 * BVH2 node, its up to eight children for BVH2 descendants (the child with the largest box is opened until the node is
 * full), every leaf child for ONE BVH2 leaf.  A node is 80 bytes = five 16-byte loads of ONE lane:
 *   child box plane k of axis a = origin[a] + q * 2^(exp[a] - 127)           (q in 0..255; lower planes rounded down,
 *                                                                              upper planes up: boxes only ever grow)
 *   slot s holds an internal child iff imask bit s; internal children are consecutive nodes from child_base in slot order
 *   leaf_valid bit 4 s + j: the leaf child in slot s has a j-th record (j < its record count <= 4); that record is
 *     recs[rec_base + number of leaf_valid bits below it]: the leaf children of one node share one contiguous run of at
 *     most 32 records, in slot order (records are ordered by wide node, breadth first)
 *   an empty slot has qlo = 255 > qhi = 0 on every axis (no ray passes its box test) and no leaf_valid bits
 * Children sit in the slot whose sign pattern (bit 0: +x, bit 1: +y, bit 2: +z) best matches the direction from the
 * node's centre to theirs, so that visiting hit slots in ascending (slot XOR ray octant) order is roughly front to back
 * without sorting distances (Ylitie, Karras, Laine: "Efficient incoherent ray traversal on GPUs through compressed wide
 * BVHs", HPG 2017 -- the node layout here is this repository's own).  Replaces what Embree's BVH4 does for the
 * reference (thirdparty/embree/kernels/bvh/bvh_intersector1.cpp:48-142). */
typedef struct TgHipWideNode {
    float    origin[3];
    uint8_t  exp[3];          /* biased exponents of the per-axis plane spacing */
    uint8_t  imask;
    uint32_t child_base;
    uint32_t rec_base;
    uint32_t leaf_valid;
    uint32_t reserved;
    uint8_t  qlo[3][8];       /* [axis][slot] */
    uint8_t  qhi[3][8];
} TgHipWideNode;              /* 80 B */
#define TGHIP_WIDE_MAX_LEAF   4    /* records per leaf child */
#define TGHIP_MAX_WIDE_DEPTH  32   /* builder guarantees depth <= this (device stack: one 8-byte entry per level) */

/* record kinds (meta >> 29) */
enum { TGHIP_REC_TRIANGLE = 0, TGHIP_REC_QUAD = 1, TGHIP_REC_CUBE = 2, TGHIP_REC_SPHERE = 3, TGHIP_REC_INSTANCE = 4,
       TGHIP_REC_DISK = 5, TGHIP_REC_CYLINDER = 6, TGHIP_REC_INSTANCE_SET = 7 };
#define TGHIP_REC_KIND(meta)   ((uint32_t)(meta) >> 29)
#define TGHIP_REC_OBJECT(meta) ((uint32_t)(meta) & 0x1FFFFFFFu)

/* 48-byte primitive record = three float4:
 *   triangle: a = v0, b = v1 - v0, c = v2 - v0                (p0,p1 unused)
 *   quad    : a = base, b = edge0, c = edge1, p0/p1 = 1/|edge0|^2, 1/|edge1|^2   (Quad.cpp:298-316)
 *   cube / sphere / disk / cylinder: geometry lives in objects[TGHIP_REC_OBJECT(meta)]; a,b,c unused
 *   instance: one rigid placement of a master mesh (primitives/Instance.cpp:290-344): a = _instancePos[i],
 *             (p0, b) = _instanceRot[i] as quaternion (w; x, y, z), c[0] = bits of the master's BVH root node index
 *             (uint32), c[1] = bits of the instance number i, c[2] = bits of the root node index of the master's wide
 *             subtree (uint32; scenes with a wide BVH); the object is the `instances` primitive.  The master's
 *             triangle records (in master space, i.e. with the master's own transform applied) and its BVH2 subtree
 *             follow the top-level ones in recs / tri_attrs / nodes and are reachable only through instance records.
 *             (ABI 8: c[1] = bits of the first inst_prims slot of the instance's leaf in the reference's tree: its box is inst_leaf_boxes[8 c[1]].)
 *   instance set (ABI 8): one `instances` primitive as the reference intersects it -- Instance::intersect walks ITS OWN BVH over
 *             the instances (bvh/BinaryBvh.hpp) and keeps the LAST hit in that tree's visiting order, each instance having
 *             been handed a ray with farT = infinity (primitives/Instance.cpp:290-311).  a = min, b = max of the primitive's
 *             bounds (BinaryBvh::_bounds), c[0] = bits of the root of the reference's tree, restated node for node by the host
 *             (csrc/host/RefInstanceBvh.cpp) and stored as ordinary TgHipBvhNode entries with the reference's exact child
 *             boxes: a node index, or -- one or two instances in all -- a leaf reference.  Leaf references of THAT tree
 *             index inst_prims[] (BinaryBvh::_primIndices: the instance records, kind TGHIP_REC_INSTANCE, of the leaf's one
 *             or two instances).  The closest-hit walk reaches the set through the scene's BVH2 (nodes[0]: over the
 *             non-instance records and the sets); the wide BVH -- walked by any-hit shadow queries, for which the order is
 *             immaterial -- holds the instance records themselves, built from their tight geometry boxes (inst_tight_boxes, below);
 *             the box of the instance's leaf in the reference's tree (inst_leaf_boxes) is tested when the record is reached. */
typedef struct TgHipPrimRec {
    float a[3]; uint32_t meta;
    float b[3]; float p0;
    float c[3]; float p1;
} TgHipPrimRec;               /* 48 B */

/* 64-byte per-triangle shading attributes, same index as the record (denormalised from the
 * reference's Vertex{pos,normal,uv}/TriangleI{v0,v1,v2,material}, primitives/Vertex.hpp:10-13,
 * Triangle.hpp:14-28, so that one hit costs one 64-B gather).  Normals are already multiplied
 * by the normal matrix (TriangleMesh.cpp:542-549). */
typedef struct TgHipTriAttr {
    float n0[3], n1[3], n2[3];
    float uv0[2], uv1[2], uv2[2];
    int32_t bsdf;             /* global bsdf index = mesh._bsdfs[clamp(tri.material)] */
} TgHipTriAttr;               /* 64 B */

/* ---- objects (one per reference Primitive) ------------------------------------------ */
enum { TGHIP_OBJ_MESH = 0, TGHIP_OBJ_QUAD = 1, TGHIP_OBJ_CUBE = 2, TGHIP_OBJ_SPHERE = 3,
       TGHIP_OBJ_INFINITE_SPHERE = 4, TGHIP_OBJ_INSTANCES = 5, TGHIP_OBJ_DISK = 6,
       TGHIP_OBJ_INFINITE_SPHERE_CAP = 7,     /* sun-like emitter: normal = _capDir, scale[0] = _cosCapAngle, edge0/edge1 = _capFrame tangent/bitangent (InfiniteSphereCap.cpp:233-249) */
       TGHIP_OBJ_POINT = 8,                   /* Dirac point light (primitives/Point.cpp): pos = _pos, scale = _power as Point.cpp:186 leaves it; never hit, sampled without random numbers */
       TGHIP_OBJ_CYLINDER = 9 };              /* primitives/Cylinder.cpp:305-319: pos = _pos, rot = _rot, normal = _axis, scale = {_radius, _halfHeight, _capped ? 1 : 0} */
#define TGHIP_OBJF_SMOOTH   1u   /* mesh "smooth": Ns interpolated (TriangleMesh.cpp:344-355) */
#define TGHIP_OBJF_SAMPLE   2u   /* infinite_sphere "sample" (InfiniteSphere.cpp:117-122)      */
#define TGHIP_OBJF_SKYDOME  4u   /* a TGHIP_OBJ_INFINITE_SPHERE that is the `skydome` primitive (primitives/Skydome.cpp): its emission is the
                                    512 x 256 sky image baked at prepareForRender (:279-306); directions map to the image without the
                                    primitive's rotation (:41-60) and chooseLight weighs it with 4 pi instead of 2 pi (:240-243) */

typedef struct TgHipObject {
    int32_t  type;            /* TGHIP_OBJ_*                                      */
    int32_t  bsdf;            /* bsdf index (quad/cube/sphere); -1 for infinite   */
    int32_t  emission;        /* texture index of the radiance, -1 = not emissive */
    int32_t  light;           /* index in lights[] if samplable emitter, else -1  */
    uint32_t flags;
    float    area, inv_area;  /* quad/cube/mesh total area                        */
    int32_t  first_light_tri; /* sampled mesh emitters: float offset of the mesh's block in light_tris, else -1 */
    float    base[3], edge0[3], edge1[3], normal[3]; /* quad (Quad.cpp:298-316)    */
    float    inv_uv_sq[2];
    float    pos[3], scale[3];                       /* cube half-extent / sphere radius in scale[0] /
                                                        disk (Disk.cpp:303-315): pos = _center, normal = _n, scale = {_r, _cosApex, -}, edge0 = _frame.tangent,
                                                        edge1 = _frame.bitangent, base = _coneBase */
    float    rot[9];                                 /* row-major 3x3 rotation (cube; infinite sphere _rotTransform) */
    float    face_cdf[3];                            /* cube (Cube.cpp:353-370)    */
    int32_t  num_light_tris;  /* sampled mesh emitters: triangles in the block (TriangleMesh::makeSamplable) */
    int32_t  int_medium, ext_medium;  /* Primitive::_intMedium/_extMedium (Primitive.cpp:30-31) as indices into media[], -1 = none;
                                         the primitive overrides the path's medium iff either is set (Primitive.hpp:172-183) */
} TgHipObject;

/* ---- BSDFs ---------------------------------------------------------------------------- */
enum { TGHIP_BSDF_LAMBERT = 0, TGHIP_BSDF_NULL = 1, TGHIP_BSDF_ROUGH_CONDUCTOR = 2,
       TGHIP_BSDF_SMOOTH_COAT = 3, TGHIP_BSDF_DIELECTRIC = 4, TGHIP_BSDF_ROUGH_DIELECTRIC = 5,
       TGHIP_BSDF_MIRROR = 6, TGHIP_BSDF_CONDUCTOR = 7, TGHIP_BSDF_PLASTIC = 8,
       TGHIP_BSDF_ROUGH_PLASTIC = 9, TGHIP_BSDF_MIXED = 10, TGHIP_BSDF_TRANSPARENCY = 11,
       TGHIP_BSDF_FORWARD = 12, TGHIP_BSDF_ERROR = 13,
       /* ABI 9: the five remaining non-fibre types of bsdfs/BsdfFactory.cpp:29-51.  Their own parameters:
        *   DIFFUSE_TRANSMISSION  eta[0] = _transmittance (0.5: the reference has no JSON key for it)
        *   PHONG                 eta[0] = _exponent, eta[1] = _diffuseRatio, k[0] = _invExponent, k[1] = _pdfFactor, k[2] = _brdfFactor (PhongBsdf.cpp:126-132)
        *   THINSHEET             ior, tex1 = _thickness (scalar texture), sigma_a, enable_refraction = _enableInterference
        *   OREN_NAYAR            roughness (scalar texture)
        *   ROUGH_COAT            ior, thickness, sigma_a, scaled_sigma_a, avg_transmittance, distribution, roughness, sub0 = _substrate */
       TGHIP_BSDF_DIFFUSE_TRANSMISSION = 14, TGHIP_BSDF_PHONG = 15, TGHIP_BSDF_THINSHEET = 16, TGHIP_BSDF_OREN_NAYAR = 17,
       TGHIP_BSDF_ROUGH_COAT = 18,
       /* Two of the factory's three fibre BCSDFs (bsdfs/LambertianFiberBcsdf.cpp, bsdfs/RoughWireBcsdf.cpp; `hair` is not restated), on ANY primitive:
        * they read the shading frame only, which -- their lobes carrying TGHIP_LOBE_ANISOTROPIC -- is the primitive's own tangent space
        * (Primitive::setupTangentFrame, Primitive.cpp:125-163; the cylinder's tangent is its axis).  Same ABI version: no struct changes, and a
        * description without them reads as before.  The kernels' type masks have no bit for them (bits 19 and 20 are scene features): the
        * all-features shading family alone evaluates them (tghip_debug_bsdf_info).  Their own parameters:
        *   LAMBERTIAN_FIBER      none (albedo); lobes = DIFFUSE_R | DIFFUSE_T | ANISOTROPIC
        *   ROUGH_WIRE            eta, k (the conductors' fields: `eta` / `k` of the JSON, or the `material` looked up, default Cu);
        *                         thickness = _v = sqr(_roughness*PI_HALF) of RoughWireBcsdf::prepareForRender (:171-174) -- `roughness` is a
        *                         plain float there, not a texture, so the texture index `roughness` stays -1; lobes = GLOSSY_R | GLOSSY_T | ANISOTROPIC */
       TGHIP_BSDF_LAMBERTIAN_FIBER = 19, TGHIP_BSDF_ROUGH_WIRE = 20 };
enum { TGHIP_DIST_BECKMANN = 0, TGHIP_DIST_PHONG = 1, TGHIP_DIST_GGX = 2 };
/* lobe bits, identical to bsdfs/BsdfLobes.hpp:13-33 */
enum { TGHIP_LOBE_GLOSSY_R = 1, TGHIP_LOBE_GLOSSY_T = 2, TGHIP_LOBE_DIFFUSE_R = 4, TGHIP_LOBE_DIFFUSE_T = 8,
       TGHIP_LOBE_SPECULAR_R = 16, TGHIP_LOBE_SPECULAR_T = 32, TGHIP_LOBE_ANISOTROPIC = 64,
       TGHIP_LOBE_FORWARD = 128 };

typedef struct TgHipBsdf {
    int32_t  type;            /* TGHIP_BSDF_*                               */
    uint32_t lobes;           /* after prepareForRender                      */
    int32_t  albedo;          /* texture index                               */
    int32_t  distribution;    /* TGHIP_DIST_*                                */
    int32_t  roughness;       /* texture index (scalar)                      */
    int32_t  sub0, sub1;      /* substrate / bsdf0,bsdf1 / base              */
    int32_t  tex1;            /* ratio / alpha texture                       */
    float    ior, thickness, avg_transmittance, diffuse_fresnel;
    int32_t  enable_refraction;
    float    eta[3], k[3], sigma_a[3], scaled_sigma_a[3];
    int32_t  bump1;           /* Bsdf::_bump (bsdfs/Bsdf.cpp:19-25, scalar request): texture index + 1 of a NON-constant bump map, 0 = none
                                 (a constant one changes nothing, Primitive.cpp:128-131); the shading frame then comes from the primitive's
                                 tangent space and the map's derivatives (Primitive::setupTangentFrame, Primitive.cpp:125-163).  (In what
                                 was padding up to ABI 7: a description written before carries 0.) */
    float    pad;
} TgHipBsdf;

/* ---- participating media (media/HomogeneousMedium.cpp) ------------------------------------------------- */
enum { TGHIP_PHASE_ISOTROPIC = 0, TGHIP_PHASE_HENYEY_GREENSTEIN = 1, TGHIP_PHASE_RAYLEIGH = 2 };   /* phasefunctions/{Isotropic,HenyeyGreenstein,Rayleigh}PhaseFunction.cpp */
/* transmittances/{Exponential,Linear,Quadratic,DoubleExponential,Pulse,Erlang,Davis,DavisWeinstein}Transmittance.cpp */
enum { TGHIP_TRANS_EXPONENTIAL = 0, TGHIP_TRANS_LINEAR = 1, TGHIP_TRANS_QUADRATIC = 2, TGHIP_TRANS_DOUBLE_EXPONENTIAL = 3,
       TGHIP_TRANS_PULSE = 4, TGHIP_TRANS_ERLANG = 5, TGHIP_TRANS_DAVIS = 6, TGHIP_TRANS_DAVIS_WEINSTEIN = 7,
       TGHIP_TRANS_INTERPOLATED = 8 };      /* InterpolatedTransmittance.cpp: trans_p = {ratio}; its two operands _trA, _trB are the trans_type / trans_p of the
                                               two media[] entries that FOLLOW this one (placeholders no primitive refers to; neither may be interpolated itself) */
typedef struct TgHipMedium {
    float   sigma_a[3], sigma_s[3], sigma_t[3];   /* after prepareForRender: material sigma x density (HomogeneousMedium.cpp:43-49) */
    int32_t absorption_only;                      /* _sigmaS == 0 */
    int32_t max_bounce;                           /* Medium::_maxBounce (Medium.cpp:16, 29) */
    int32_t phase_type;                           /* TGHIP_PHASE_* */
    float   phase_g;                              /* Henyey-Greenstein asymmetry */
    int32_t trans_type;                           /* TGHIP_TRANS_*: Medium::_transmittance (Medium.cpp:14, 27-28) */
    float   trans_p[3];                           /* linear / quadratic: {max_t}; double_exponential: {sigma_a, sigma_b}; pulse: {min, max, num_pulses};
                                                     erlang: {rate}; davis: {alpha}; davis_weinstein: {h, c} */
    /* ABI 9: media/ExponentialMedium.cpp next to the homogeneous medium -- the density falls off as exp(-falloff_scale (p - unit_point) . falloff_dir);
       sigma_* are the medium's coefficients at density one; exponential transmittance only (ExponentialMedium::sampleDistance hands the
       transmittance's eval an `exited` flag it has not set yet, :122-123: only the exponential one does not look at it) */
    int32_t medium_type;                          /* TGHIP_MEDIUM_* */
    float   falloff_scale;                        /* _falloffScale */
    float   unit_point[3];                        /* _unitPoint */
    float   falloff_dir[3];                       /* _unitFalloffDirection (normalised at prepareForRender) */
    float   pad[3];
} TgHipMedium;                /* 112 B */
/* media/AtmosphericMedium.cpp (TGHIP_MEDIUM_ATMOSPHERE): density exp(-s^2 (|p - center|^2 - radius^2)); the fields above are reused --
   falloff_scale = s = _effectiveFalloffScale (falloff_scale / radius after prepareForRender, :79), unit_point = _center (the pivot primitive's
   origin when the scene names one, :70-77), falloff_dir[0] = _radius; exponential transmittance only, for the reason given for the exponential
   medium (AtmosphericMedium::sampleDistance, :150-151) */
enum { TGHIP_MEDIUM_HOMOGENEOUS = 0, TGHIP_MEDIUM_EXPONENTIAL = 1, TGHIP_MEDIUM_ATMOSPHERE = 2 };

/* ---- textures ------------------------------------------------------------------------- */
/* textures/TextureFactory.cpp:11-18.  An `ies` texture (textures/IesTexture.cpp) is a scalar bitmap the host bakes at load: it arrives as TGHIP_TEX_BITMAP.
 * TGHIP_TEX_DISK  (textures/DiskTexture.cpp):  value = _value; every other field unused.
 * TGHIP_TEX_BLADE (textures/BladeTexture.cpp): value = _value and, in fields the type does not otherwise use, what BladeTexture::init (:22-31) leaves:
 *     res_u = _numBlades          scale = _angle
 *     on_color[0] = _bladeAngle   on_color[1] = _area        on_color[2] = 1.0f/_area (the pdf inside the polygon)
 *     off_color[0], [1] = _baseNormal                        off_color[2], pad = _baseEdge
 * Both are evaluated by the all-features shading family only (a scene that holds one is shaded by it throughout).
 * Where a texture is SAMPLED -- the emission of a sampled infinite_sphere (primitives/InfiniteSphere.cpp:161-176, 218-229) and a thin lens's aperture
 * (TgHipCamera) --, every type goes through its own sample / pdf: a bitmap through its Distribution2D (dist_offset), disk and blade as above, a
 * TGHIP_TEX_CHECKER through CheckerTexture::sample / pdf (textures/CheckerTexture.cpp:85-123) from on_color, off_color, res_u and res_v as they are --
 * in the all-features family again: a scene whose sampled infinite_sphere has a checker emission is shaded by it throughout --, a constant uniformly. */
enum { TGHIP_TEX_CONSTANT = 0, TGHIP_TEX_CHECKER = 1, TGHIP_TEX_BITMAP = 2, TGHIP_TEX_DISK = 3, TGHIP_TEX_BLADE = 4 };
#define TGHIP_TEXF_LINEAR 1u
#define TGHIP_TEXF_CLAMP  2u
#define TGHIP_TEXF_RGB    4u
#define TGHIP_TEXF_VALID  8u

typedef struct TgHipTexture {
    int32_t  type;
    uint32_t flags;
    int32_t  w, h;
    float    value[3];        /* constant value                              */
    float    scale;           /* bitmap _scale                               */
    float    on_color[3];  int32_t res_u;
    float    off_color[3]; int32_t res_v;
    float    avg[3];          /* Texture::average()                          */
    float    pad;
    int64_t  texel_offset;    /* float offset into texels (3 per texel if RGB, else 1) */
    int64_t  dist_offset;     /* float offset into dist: marginalPdf[h] marginalCdf[h+1] pdf[w*h] cdf[(w+1)*h]; -1 = none
                                 (sampling/Distribution2D.hpp:18-83 built by BitmapTexture::makeSamplable, BitmapTexture.cpp:400-431) */
} TgHipTexture;

/* ---- camera (cameras/PinholeCamera.cpp:28-86, Camera.cpp:44-68, ReconstructionFilter) ---- */
enum { TGHIP_FILTER_DIRAC = 0, TGHIP_FILTER_BOX = 1, TGHIP_FILTER_TABULATED = 2 };
enum { TGHIP_CAMERA_PINHOLE = 0, TGHIP_CAMERA_THINLENS = 1,     /* cameras/PinholeCamera.cpp, cameras/ThinlensCamera.cpp */
       TGHIP_CAMERA_EQUIRECTANGULAR = 2,   /* cameras/EquirectangularCamera.cpp: the full sphere around pos, longitude across the image, latitude down it;
                                              inv_xf[0..8] then holds _rot = _transform.extractRotation() row-major (EquirectangularCamera.cpp:129-134) and
                                              inv_xf[9] = 1 / res_y (Camera::_pixelSize.y; pixel_size_x = 1 / res_x as for every camera) */
       TGHIP_CAMERA_CUBEMAP = 3 };         /* cameras/CubemapCamera.cpp: six 90-degree faces laid out as a cross, a row or a column; inv_xf as for the
                                              equirectangular camera, blade_count = CubemapCamera::ProjectionMode (0 horizontal_cross, 1 vertical_cross, 2 row, 3 column) */
enum { TGHIP_APERTURE_DISK = 0, TGHIP_APERTURE_BLADE = 1,       /* textures/DiskTexture.cpp:78-81, textures/BladeTexture.cpp:110-130 */
       TGHIP_APERTURE_BITMAP = 2,                               /* textures/BitmapTexture.cpp:433-439 with the MAP_UNIFORM distribution (:400-431); an `ies`
                                                                   aperture too: IesTexture is a BitmapTexture and its bake is what makeSamplable weighs */
       /* (3 is no aperture and stays refused) */
       TGHIP_APERTURE_CONSTANT = 4,                             /* textures/ConstantTexture.cpp:69-72: the lens sample as it is, a square aperture */
       TGHIP_APERTURE_CHECKER = 5 };                            /* textures/CheckerTexture.cpp:85-112: aperture_w = _resU, aperture_h = _resV,
                                                                   blade_edge[0] = _onColor.max(), blade_edge[1] = _offColor.max() (finite, not negative,
                                                                   not both zero: a checker of two blacks samples like TGHIP_APERTURE_CONSTANT, :88-91, and
                                                                   is flattened as that) */
typedef struct TgHipCamera {
    float   pos[3];
    float   plane_dist;
    float   xf[9];            /* row-major upper 3x3 of Camera::_transform (right axis negated) */
    float   ratio, pixel_size_x;
    int32_t res_x, res_y;
    int32_t filter_type;
    float   filter_width, filter_bin_size;
    float   filter_cdf[32];   /* ReconstructionFilter::_cdf (RFILTER_RESOLUTION = 31) */
    /* thin lens (cameras/ThinlensCamera.cpp:85-126); the aperture texture is only ever sampled by the forward path tracer
     * (samplePosition, :85-97): the default disk (textures/DiskTexture.cpp:78-86), an n-blade polygon (BladeTexture.cpp:21-31, 110-130), a
     * bitmap or an IES bake (BitmapTexture::sample), a constant or a checker -- every texture type the reference's factory makes.  A checker's
     * parameters ride in fields its type does not otherwise use (TGHIP_APERTURE_CHECKER above); the struct keeps its size */
    int32_t type;             /* TGHIP_CAMERA_*                                   */
    float   focus_dist, aperture_size, cat_eye;
    float   inv_xf[12];       /* rows 0..2 of Camera::_invTransform (3x4, row-major, translation in column 3) */
    int32_t medium;           /* Camera::_medium (Camera.cpp:49-50): index into media[], -1 = none */
    int32_t aperture_type;    /* TGHIP_APERTURE_*                                  */
    int32_t blade_count;      /* BladeTexture::_numBlades                          */
    float   blade_angle, blade_step;   /* _angle, _bladeAngle = 2 pi / blades     */
    float   blade_edge[2];    /* _baseEdge                                         */
    /* TGHIP_APERTURE_BITMAP: the aperture bitmap's Distribution2D (ThinlensCamera::precompute makes it samplable with MAP_UNIFORM,
     * cameras/ThinlensCamera.cpp:27-35): its size and the float offset of its tables in dist[], laid out like TgHipTexture::dist_offset's */
    int32_t  aperture_w, aperture_h;
    uint32_t aperture_dist;
} TgHipCamera;

/* ---- integrator settings (TraceSettings.hpp:23-39, PathTracerSettings.hpp:25-43) -------- */
typedef struct TgHipSettings {
    int32_t min_bounces, max_bounces;
    int32_t enable_light_sampling, enable_two_sided_shading, enable_consistency_checks;
    int32_t enable_volume_light_sampling;   /* PathTracerSettings.hpp:13,38; low_order_scattering / include_surfaces must keep their defaults (true) */
    int32_t pad[2];
} TgHipSettings;

typedef struct TgHipSceneDesc {
    uint32_t abi_version;     /* TGHIP_ABI_VERSION */
    uint32_t num_nodes, num_recs, num_objects, num_lights, num_infinite_lights, num_bsdfs, num_textures;
    const TgHipBvhNode *nodes;
    const TgHipPrimRec *recs;
    const TgHipTriAttr *tri_attrs;        /* num_recs entries (unused for non-triangles) */
    const TgHipObject  *objects;
    const int32_t      *lights;           /* object indices, TraceableScene::_lights order (TraceableScene.hpp:86-102) */
    const int32_t      *infinite_lights;  /* object indices, TraceableScene::_infiniteLights */
    const TgHipBsdf    *bsdfs;
    const TgHipTexture *textures;
    const float        *texels;  uint64_t num_texel_floats;
    const float        *dist;    uint64_t num_dist_floats;
    /* sampled mesh emitters (TriangleMesh.cpp:395-409): per mesh a block of floats at objects[].first_light_tri:
     * cdf[n + 1] of the triangle areas (Distribution1D: normalised, last = 1), then n x 9 floats p0,p1,p2 (world space,
     * the mesh's own triangle order); objects[].area is the total area */
    const float        *light_tris;  uint64_t num_light_tri_floats;
    /* generator matrices of the Sobol' sequence, TGHIP_SOBOL_DIMS x TGHIP_SOBOL_BITS words -- the host's own copy of
     * sobol::Matrices::matrices (thirdparty/sobol/sobol.h:30-35); NULL/0 unless passes use TGHIP_PASS_SOBOL */
    const uint32_t     *sobol_matrices;  uint64_t num_sobol_words;
    uint32_t num_instances;               /* instance records among recs (0: single-level scene) */
    uint32_t num_top_recs;                /* top-level records = recs[0, num_top_recs): the non-instance and the instance records in the
                                             wide BVH's order, then the instance-set records; the rest belong to masters */
    /* ABI 8, scenes with instances: the leaf slots of the reference's instance trees (see the instance-set record) -> instance record,
     * and, at a leaf's FIRST slot, the leaf's box as its parent stores it: lo[3], pad, hi[3], pad -- two 16-byte loads; the root's bounds
     * for a tree that is one leaf; num_inst_prims entries, the second slot of a two-instance leaf unused */
    const uint32_t     *inst_prims;       uint32_t num_inst_prims;
    const float        *inst_leaf_boxes;
    /* ... and per top-level record that is an instance (indexed by the record: 8 floats at 8 x record index, num_top_recs entries, the
     * others zero) a box -- lo[3], pad, hi[3], pad -- that holds the instance's geometry in world space and lies inside the reference's
     * box of the instance: a ray that misses it cannot hit the instance, so its master is not walked (an optimisation only: the
     * reference walks it and finds nothing).  The wide BVH is built from these boxes. */
    const float        *inst_tight_boxes;
    const TgHipMedium  *media;  uint32_t num_media;   /* Scene::_media; NULL/0 = the scene has no participating media */
    /* the wide BVH: wide_nodes[0] is the root of the tree over recs[0, num_top_recs); with instances every master's wide
     * subtree follows (its root in the instance records' c[2]).  NULL/0 = the device walks the BVH2 (flat-list scenes do) */
    const TgHipWideNode *wide_nodes;  uint32_t num_wide_nodes;
    /* the reference's top-level Embree tree over the records of a flat list of analytic primitives (TgHipTopNode; ABI 10); NULL / 0 otherwise */
    const TgHipTopNode *top_nodes;  uint32_t num_top_nodes;
    TgHipCamera   camera;
    TgHipSettings settings;
    float         bounds_lo[3], bounds_hi[3];
} TgHipSceneDesc;

/* ---- passes ------------------------------------------------------------------------------
 * A pass renders samples [spp_begin, spp_end) of every pixel owned by this shard.  Ownership
 * follows the reference's 16x16 tile dicing (PathTraceIntegrator.cpp:27-42): tile (tx, ty) belongs to
 * shard tghip_tile_owner(tx, ty, shard_count) = (tx + ty*skew) % shard_count -- a diagonal interleave, so
 * that a shard's tiles are spread over the image in x AND y whatever the image width (plain t % N over
 * row-major tiles degenerates into N vertical stripes whenever the tiles per row are a multiple of N:
 * 1280, 1920 and 3840 pixels all are for N = 8); a shard renders its tiles in row-major order.  Random
 * numbers are a counter-based PCG stream keyed by (seed, pixelIndex, sampleIndex) -- see DESIGN.md "RNG". */
static inline uint32_t tghip_shard_skew(uint32_t shard_count)      /* the smallest odd prime that does not divide shard_count */
{
    static const uint32_t primes[6] = {3u, 5u, 7u, 11u, 13u, 17u};
    for (int i = 0; i < 6; ++i)
        if (shard_count % primes[i] != 0u)
            return primes[i];
    return 1u;
}
static inline uint32_t tghip_tile_owner(uint32_t tx, uint32_t ty, uint32_t shard_count)
{
    return shard_count <= 1u ? 0u : (tx + ty*tghip_shard_skew(shard_count)) % shard_count;
}
#define TGHIP_SOBOL_DIMS 1024u
#define TGHIP_SOBOL_BITS 52u
#define TGHIP_TILE_SIZE 16u              /* PathTraceIntegrator::TileSize */
#define TGHIP_VARIANCE_TILE_SIZE 4u      /* PathTraceIntegrator::VarianceTileSize: one SampleRecord per 4x4 pixels */
/* pass flags */
#define TGHIP_PASS_SOBOL   1u   /* next1D/next2D come from the scrambled Sobol' sequence exactly as SobolPathSampler does
                                   (sampling/SobolPathSampler.hpp:20-79: scramble = tile seed ^ hash32(pixel), permuted index,
                                   one dimension per draw up to 1024); booleans and later dimensions come from the
                                   counter-based PCG stream (the reference uses a sequential per-tile stream there) */
#define TGHIP_PASS_RECORDS 2u   /* keep the per-4x4-pixel SampleRecords (path_tracer/SampleRecord.hpp:46-65) up to date */

#define TGHIP_PASS_AUX     4u   /* keep the auxiliary output buffers (TgHipAuxPixel) up to date: depth / normal / albedo / visibility of the
                                   first non-specular vertex (PathTracer.cpp:78-96, 133-140) and the colour, each with its A/B halves and
                                   sample variance (cameras/OutputBuffer.hpp:90-132) */

#define TGHIP_PASS_SAMPLES 8u   /* parity instrumentation: additionally keep the radiance of every individual sample of the pass -- the
                                   return value of PathTracer::traceSample (PathTracer.cpp:14-149) for (pixel, sample index) -- in a
                                   device buffer read back with tghip_download_samples; not with record_index / record_count */

/* auxiliary outputs (cameras/OutputBufferSettings.cpp:8-14) and their channels in TgHipAuxPixel */
enum { TGHIP_AUX_COLOR = 0, TGHIP_AUX_DEPTH = 1, TGHIP_AUX_NORMAL = 2, TGHIP_AUX_ALBEDO = 3, TGHIP_AUX_VISIBILITY = 4, TGHIP_AUX_OUTPUTS = 5 };
#define TGHIP_AUX_CHANNELS 11u   /* color rgb 0-2 | depth 3 | normal xyz 4-6 | albedo rgb 7-9 | visibility 10 */
/* OutputBuffer state of one pixel for all five outputs, kept as if two_buffer_variance and sample_variance were both on
 * (OutputBuffer.hpp:90-132: _bufferA = running mean of the samples with even index, _bufferB = odd, _variance = Welford sum
 * against the mean of both, _sampleCount per output -- an output skips the samples that did not record it).  The host
 * derives what a scene's OutputBufferSettings ask for: mean = (A nA + B nB)/n. */
typedef struct TgHipAuxPixel {
    float    a[11], b[11], variance[11];
    uint32_t count[5];
} TgHipAuxPixel;              /* 152 B */

/* the device-resident part of SampleRecord: Welford mean / running variance of the sample luminance,
 * accumulated in the reference's order (tile row-major pixel order, then sample index: PathTraceIntegrator.cpp:136-156) */
typedef struct TgHipSampleRecord { uint32_t sample_count; float mean, running_variance; } TgHipSampleRecord;

typedef struct TgHipPassDesc {
    uint32_t spp_begin, spp_end;
    uint32_t seed;
    uint32_t shard_index, shard_count;   /* 0,1 = whole image */
    uint32_t flags;                      /* TGHIP_PASS_* */
    /* host arrays, borrowed until tghip_wait returns; NULL when unused */
    const uint32_t *tile_seeds;          /* TGHIP_PASS_SOBOL: SobolPathSampler seed per 16x16 tile, dice order */
    const uint32_t *record_index;        /* adaptive sampling: per SampleRecord (ceil(W/4) x ceil(H/4), row-major) the first */
    const uint32_t *record_count;        /*   sample index and the samples per pixel of this pass; then spp_begin/spp_end are ignored */
} TgHipPassDesc;

typedef struct TgHipCounters {
    uint64_t samples;           /* camera paths completed                         */
    uint64_t closest_rays;      /* closest-hit queries (extension rays)           */
    uint64_t shadow_rays;       /* shadow-type closest-hit queries                */
    uint64_t nodes_visited;     /* BVH nodes fetched, all rays (0 unless counting is enabled) */
    uint64_t prims_tested;      /* primitive records tested, all rays                          */
    uint64_t iterations;        /* wavefront iterations                           */
    double   ms_trace_closest, ms_trace_shadow, ms_shade, ms_other, ms_total;  /* HIP-event time, last pass set */
    uint64_t launches_trace_closest, launches_trace_shadow, launches_shade;
    uint64_t nodes_visited_shadow; /* the shadow-ray share of nodes_visited / prims_tested (counting enabled) */
    uint64_t prims_tested_shadow;
    uint64_t shadow_slots;         /* path vertices that queued at least one shadow ray */
    uint64_t tail_launches;        /* batches whose last paths ran in the single-launch tail kernel (k_tail) */
} TgHipCounters;

/* closest-hit query record for tghip_trace_rays (and the oracle's equivalent) */
typedef struct TgHipRay { float o[3], tmin, d[3], tmax; } TgHipRay;          /* 32 B */
typedef struct TgHipHit { float t, u, v; int32_t rec; } TgHipHit;            /* 16 B; rec = -1 on miss */

typedef struct tghip_ctx tghip_ctx;

tghip_ctx  *tghip_create(int device_ordinal);
void        tghip_destroy(tghip_ctx *ctx);
const char *tghip_last_error(tghip_ctx *ctx);      /* ctx may be NULL: last create error */
int         tghip_device_count(void);

/* A description that is refused (TGHIP_E_INVALID / TGHIP_E_UNSUPPORTED: malformed, or outside what the device code supports) leaves the context exactly as it
 * was: the scene uploaded before stays uploaded and renders on.  Every such refusal is decided on the host before the device is touched, by the check
 * tgh_scene_check (tungsten_host.h) runs on its own. */
int tghip_upload_scene(tghip_ctx *ctx, const TgHipSceneDesc *scene);
int tghip_render_pass(tghip_ctx *ctx, const TgHipPassDesc *pass);   /* asynchronous */
int tghip_wait(tghip_ctx *ctx);
int tghip_abort(tghip_ctx *ctx);
int tghip_clear_framebuffer(tghip_ctx *ctx);
/* Use caller-owned DEVICE buffers (e.g. a torch tensor) as framebuffer: sum = W*H*3 floats,
 * count = W*H uint32.  Pass NULLs to go back to the internal buffers. */
int tghip_bind_framebuffer(tghip_ctx *ctx, float *dev_rgb_sum, uint32_t *dev_count);
int tghip_download_framebuffer(tghip_ctx *ctx, float *rgb_sum, uint32_t *count, size_t npixels);
/* restores a saved framebuffer (OutputBuffer::deserialize, cameras/OutputBuffer.hpp:191-200): resume of an interrupted render */
int tghip_upload_framebuffer(tghip_ctx *ctx, const float *rgb_sum, const uint32_t *count, size_t npixels);
/* SampleRecords (TGHIP_PASS_RECORDS): n = ceil(W/4)*ceil(H/4); cleared by tghip_clear_framebuffer.  Records of tiles
 * this context never rendered stay zero; upload restores a resumed / merged state. */
int tghip_download_records(tghip_ctx *ctx, TgHipSampleRecord *out, size_t n);
int tghip_upload_records(tghip_ctx *ctx, const TgHipSampleRecord *in, size_t n);
/* auxiliary output buffers (TGHIP_PASS_AUX), one TgHipAuxPixel per image pixel; allocated by the first TGHIP_PASS_AUX pass,
 * cleared by tghip_clear_framebuffer (Camera::serializeOutputBuffers / deserializeOutputBuffers, Camera.cpp:222-238) */
int tghip_download_aux(tghip_ctx *ctx, TgHipAuxPixel *out, size_t npixels);
int tghip_upload_aux(tghip_ctx *ctx, const TgHipAuxPixel *in, size_t npixels);
/* the per-sample radiance of the last TGHIP_PASS_SAMPLES pass: nfloats = W*H*(spp_end - spp_begin)*3, laid out
 * [pixel (row-major)][sample - spp_begin][rgb]; samples of pixels the pass's shard does not own are zero */
int tghip_download_samples(tghip_ctx *ctx, float *rgb, size_t nfloats);
/* Develops the frame where it lives: the images Integrator::writeBuffers and Camera::saveOutputBuffers put into files (integrators/Integrator.cpp:56-80,
 * cameras/OutputBuffer.hpp:56-86, 134-189), computed by kernels of their own (csrc/hip/develop.hip) from the framebuffer -- the bound one when one is
 * bound -- or from the auxiliary output buffers, bit for bit what the host computes from a download (tungsten_host.h: tgh_develop_host_frame / _aux).
 *   source  TGHIP_DEVELOP_FRAME: mean = sum * (count ? 1 / count : 0); the 8-bit image is max(mean, 0) under one of the operators of
 *           cameras/Tonemap.hpp:25-48 (powf as glibc computes it), times 255, converted as x86 converts (NaN and everything outside int32
 *           become INT_MIN, so 0 -- not the 255 a saturating conversion gives), clamped to [0, 255];
 *           a TGHIP_AUX_* output: part = the combined mean (a nA + b nB)/max(n, 1), the A or B half, or variance/(n max(1, n - 1)); the 8-bit image
 *           as OutputBuffer::saveLdr makes it: depth divided by the image's largest entry that is not +inf (0 when there is none; a NaN never wins),
 *           normals mapped from [-1, 1], the variance part and the other outputs as they are, a pixel whose channel average is NaN or infinite
 *           white, one channel replicated to three; never tone-mapped (`tonemap` is ignored);
 *   hdr_out 3 floats per pixel for the frame, the output's channel count (3, 1, 3, 3, 1) otherwise; ldr_out 3 bytes per pixel.  Either may be NULL.
 *           Host memory, or with TGHIP_DEVELOP_DEVICE_POINTERS memory of the context's device (hdr_out 16-byte, ldr_out 4-byte aligned).
 * Waits for the running pass like the download calls.  TGHIP_E_INVALID: NULL context or description, unknown source / part / operator, npixels != W*H,
 * an aux source before any aux buffer exists, a part other than the mean of the frame.  TGHIP_E_UNSUPPORTED: the context's "develop_host" option is
 * set -- the caller develops on the host (the host integrator does; its files are the same bytes either way). */
enum { TGHIP_TONEMAP_LINEAR = 0, TGHIP_TONEMAP_GAMMA = 1, TGHIP_TONEMAP_REINHARD = 2, TGHIP_TONEMAP_FILMIC = 3, TGHIP_TONEMAP_PBRT = 4 };
enum { TGHIP_DEVELOP_MEAN = 0, TGHIP_DEVELOP_A = 1, TGHIP_DEVELOP_B = 2, TGHIP_DEVELOP_VARIANCE = 3 };
#define TGHIP_DEVELOP_FRAME 0xffffffffu       /* source: the framebuffer; otherwise a TGHIP_AUX_* output */
#define TGHIP_DEVELOP_DEVICE_POINTERS 1u      /* flags: out pointers are device memory (a torch tensor) */
typedef struct TgHipDevelopDesc { uint32_t source, part, tonemap, flags; } TgHipDevelopDesc;
int tghip_develop(tghip_ctx *ctx, const TgHipDevelopDesc *desc, float *hdr_out, uint8_t *ldr_out, size_t npixels);
/* Instrumentation: HIP-event time of the kernels of the context's last tghip_develop, in milliseconds (profiles/r8_develop.txt) */
int tghip_develop_kernel_time(tghip_ctx *ctx, double *ms);
/* The denoiser's NL-means filter (denoiser/NlMeans.hpp:95-157: nlMeans with nlMeansWeights :47-93 and denoiser/BoxFilter.hpp) on the device, by
 * kernels of its own (csrc/hip/denoise.hip): out = the `image` filtered with weights from `guide` and `variance`, patch radius F, search radius R,
 * distance scale k, the variance times variance_scale -- float32, operation for operation in the reference's order (32 x 32 tiles, offsets dy outer and dx
 * inner, the box filter's running sums and its in-place slow path in narrow rectangles), so the bits are the reference's and the host's
 * (tungsten_host.h: tgh_nlmeans_host).  A C-channel image is C independent scalar filters, as nlMeans<Vec3f> and SimdNlMeans' float4 are.
 *   source  TGHIP_NLMEANS_POINTERS: image / guide / variance / out are height x width pixels of `channels` interleaved floats -- host memory, or with
 *           TGHIP_DEVELOP_DEVICE_POINTERS memory of the context's device (4-byte aligned); no scene is needed;
 *           a TGHIP_AUX_* output: image, guide and variance are NULL, and the three planes are the float images tghip_develop gives for that output's
 *           image_part, guide_part and TGHIP_DEVELOP_VARIANCE, developed on the device into scratch; `channels` is set by the output (3, 1, 3, 3, 1:
 *           the description's value is ignored) and width x height must be the frame's.  NFOR's feature prefilter of an output is two calls:
 *           image A with guide B and image B with guide A, F 3, R 5, k 0.5, variance_scale 2.
 * Non-finite input pixels are outside the contract: what the reference's float-to-int conversion and its min / max make of a NaN is not restated.
 * Waits for the running pass like tghip_develop.  TGHIP_E_INVALID (tghip_last_error says which): NULL context or description, channels outside
 * 1..4, F above 8, R above 16, k <= 0, a zero dimension, an unknown source or part, an aux source before an aux buffer exists or with another size
 * than the frame's, pointers given with an aux source, pointers missing without one. */
#define TGHIP_NLMEANS_POINTERS 0xffffffffu    /* source: the caller's arrays; otherwise a TGHIP_AUX_* output of the context */
typedef struct TgHipNlMeansDesc {
    uint32_t width, height, channels;   /* 1..4, interleaved */
    uint32_t F, R;                      /* patch and search radius */
    float    k, variance_scale;
    uint32_t source;                    /* TGHIP_NLMEANS_POINTERS, or a TGHIP_AUX_* output of the context */
    uint32_t image_part, guide_part;    /* with an aux source: TGHIP_DEVELOP_MEAN / _A / _B */
    uint32_t flags;                     /* TGHIP_DEVELOP_DEVICE_POINTERS: all pointers are memory of the context's device */
} TgHipNlMeansDesc;
int tghip_nlmeans(tghip_ctx *ctx, const TgHipNlMeansDesc *desc, const float *image, const float *guide, const float *variance, float *out);
/* Instrumentation: HIP-event time of the kernels of the context's last tghip_nlmeans (the develop kernels of an aux source included), in
 * milliseconds (profiles/r9_denoise.txt) */
int tghip_nlmeans_kernel_time(tghip_ctx *ctx, double *ms);
/* Multi-GPU framebuffer merge inside one process: ctxs[0..n) are the contexts (one per device, all with the same scene
 * uploaded) that rendered the tile shards 0..n-1 of a frame (TgHipPassDesc.shard_index/shard_count).  Their radiance sums
 * (float32) and sample counts (uint32) are sum-reduced by RCCL (ncclReduce over xGMI, one communicator per device, created at
 * the first call and kept) into a scratch buffer on ctxs[root]'s device and copied from there into rgb_sum / count (host,
 * npixels = W*H; either may be NULL).  Tile ownership is disjoint, so the sums are exact (x + 0) in any reduction order; the
 * contexts' own framebuffers are left as they are, so passes can go on accumulating.  librccl.so is loaded at the first call;
 * TGHIP_E_UNSUPPORTED when it is missing. */
int tghip_reduce_framebuffers(tghip_ctx *const *ctxs, int n, int root, float *rgb_sum, uint32_t *count, size_t npixels);
/* The same merge between PROCESSES, one per GPU (how `python -m torch.distributed.run --nproc-per-node N` / mpirun deploy it; the reference's
 * analogue is one `tungsten` process per machine and `hdrmanip --merge` over their output files, src/hdrmanip/hdrmanip.cpp:69-112):
 *   rank 0:     tghip_comm_unique_id(id, TGHIP_COMM_ID_BYTES)  -- ncclGetUniqueId; the caller carries the bytes to the other ranks by any means it
 *               has (a file, a socket, MPI_Bcast, torch.distributed.broadcast_object_list);
 *   every rank: tghip_comm_init_rank(ctx, id, bytes, nranks, rank)  -- collective: ncclCommInitRank on ctx's device; the communicator belongs to
 *               the context and is destroyed with it;
 *   every rank: tghip_reduce_framebuffer_rank(ctx, root, rgb_sum, count, npixels)  -- collective: waits for ctx's pass, then ncclReduce (sum) of the
 *               radiance sums and sample counts of every rank's framebuffer -- rank r rendered shard r of `nranks`, TgHipPassDesc.shard_* -- into a
 *               scratch image on the root's device; on the root that image is copied to rgb_sum / count (host; either may be NULL: the reduced
 *               image then stays in HBM), the other ranks pass NULL.  Exact for the same reason as above; framebuffers are left as they are. */
#define TGHIP_COMM_ID_BYTES 128
int tghip_comm_unique_id(void *id, size_t bytes);
int tghip_comm_init_rank(tghip_ctx *ctx, const void *id, size_t bytes, int nranks, int rank);
int tghip_reduce_framebuffer_rank(tghip_ctx *ctx, int root, float *rgb_sum, uint32_t *count, size_t npixels);
int tghip_trace_rays(tghip_ctx *ctx, const TgHipRay *rays, TgHipHit *hits, size_t n, int repeats, double *ms_per_launch);
/* Batched ray queries against the uploaded scene (TraceableScene::intersect and ::occluded, renderer/TraceableScene.hpp:170-223), on host memory or on
 * memory of the context's device, by kernels of their own (csrc/hip/ray_query.hip: persistent workgroups that claim rays from one counter as their
 * lanes fall idle).
 *   mode    TGHIP_QUERY_CLOSEST: out = n TgHipHit; for every ray what tghip_trace_rays returns on the same context -- rec, and on a hit t, u, v, bit
 *           for bit -- in every kind of scene (flat list with or without the top-level tree, BVH2, 8-wide BVH, `instances` in the reference's
 *           visiting order).  Infinite emitters are never hit.
 *           TGHIP_QUERY_OCCLUDED: out = n bytes, 1 exactly when the closest-hit query of the same ray has rec >= 0, else 0: the closest-hit
 *           formulation of the path tracer's shadow rays (TraceBase.cpp:79, 114-115) over geometry only -- no light is left out, nothing is
 *           transparent; not the primitives' own `occluded` routines.
 *   flags   0: rays and out are host memory (staged through buffers of the context that only grow); TGHIP_DEVELOP_DEVICE_POINTERS: both are memory
 *           of the context's device, rays and hits 16-byte aligned, occlusion bytes unaligned.
 * A ray with a non-finite component or a zero direction gets an unspecified answer; the call returns.  Runs on the context's stream, waits for a
 * running pass like tghip_develop, returns when the answers are complete (device memory: the kernel has finished, the caller's streams need no
 * further synchronisation) and allocates nothing per call.  n == 0 succeeds.  TGHIP_E_NOSCENE without an upload.  TGHIP_E_INVALID, the context still
 * usable: no description, NULL rays or out with n > 0, an unknown mode, unknown flag bits, non-zero reserved words, n > 2^31 - 1, misaligned device
 * pointers (tungsten_host.h: tgh_query_rays_check is the same check on its own).  The options "query_blocks" (workgroups; 0 = the measured default)
 * and "query_refill_at" (1..64: idle lanes of a wave at which it claims; 0 = the measured default) steer the kernel and never change an answer.
 * tghip_trace_rays and its exact visit counts stay as they are; these queries count no visits. */
enum { TGHIP_QUERY_CLOSEST = 0, TGHIP_QUERY_OCCLUDED = 1 };
typedef struct TgHipRayQueryDesc { uint32_t mode, flags, reserved[2]; } TgHipRayQueryDesc;   /* flags: TGHIP_DEVELOP_DEVICE_POINTERS */
int tghip_query_rays(tghip_ctx *ctx, const TgHipRayQueryDesc *desc, const TgHipRay *rays, void *out, size_t n);
/* Instrumentation: HIP-event time of the kernel of the context's last tghip_query_rays, in milliseconds (profiles/ray_query_ab.txt) */
int tghip_query_rays_kernel_time(tghip_ctx *ctx, double *ms);
/* Radiance along caller-supplied rays: for ray i and every sample index s of [spp_begin, spp_end) one PathTracer::traceSample
 * (integrators/path_tracer/PathTracer.cpp:14-149) from the point BEHIND the camera -- behind Camera::sampleDirection (:22-28) --, by the wavefront loop of
 * tghip_render_pass / tghip_wait itself: a pass over a virtual image whose pixel i is ray i, with a small launch of its own (csrc/hip/radiance_query.hip:
 * k_query_paths) in front of every closest-hit launch that puts the caller's ray where the camera's would be, and one behind it (k_query_clip) that ends
 * the ray's first segment at its tmax.
 *   path start   throughput 1, bounce 0, wasSpecular true (PathTracer.cpp:35-45: an emitter the ray hits directly is seen), in the medium the scene's
 *                camera is in (Camera::_medium, :38-41); the first segment is [rays[i].tmin, rays[i].tmax) (the camera's ray has 1e-4 and infinity,
 *                math/Ray.hpp:24), its end exact: a hit at t counts when t < tmax, whatever the walk's own arithmetic makes of a far distance a
 *                few ulps from a hit (the walk looks 2^-10 further and k_query_clip, behind every closest-hit launch, turns a hit at t >= tmax into
 *                a miss; tmin is the walk's near distance as it is); a ray that hits nothing inside it ends as
 *                an escaped path does: the infinite emitters are evaluated under the usual
 *                rule (TraceBase::handleInfiniteLights, integrators/TraceBase.cpp:573-590).  Everything behind the start is the loop as it is: next-event
 *                estimation and MIS, media, roulette, the NaN guards, min_bounces / max_bounces and every other integrator setting of the uploaded scene.
 *   numbers      ray i, sample s draws from the counter-based stream keyed (seed, i, s) -- the ray index where a pass has the pixel index -- from its
 *                THIRD number on: numbers 0 and 1 are the two a pinhole camera spends on its pixel filter (cameras/PinholeCamera.cpp:70-86).  With
 *                TGHIP_RADIANCE_SOBOL the path starts at Sobol' dimension 2 of the sampler TGHIP_PASS_SOBOL describes, its scramble sobol_seed ^ hash32(i)
 *                (sampling/SobolPathSampler.hpp:47-52: every ray's "tile" has the seed sobol_seed).  So a query on a pinhole camera's own rays, in pixel
 *                order, returns that camera's samples bit for bit.  The scene's camera TYPE changes nothing: on a thin-lens scene no lens point is drawn, on
 *                an equirectangular or cubemap scene k_camera_rays does not run.
 *   result       rgb_sum[3 i ..] = the float32 sum of the ray's samples, added one by one in sample-index order starting from zero (a query's work
 *                items hold one sample each and are summed without a pass's groups of four); count[i] = the samples counted; both as OutputBuffer::addSample
 *                keeps the framebuffer (cameras/OutputBuffer.hpp:104-132, PathTracer.cpp:130-131): a NaN radiance is a black sample that counts, an
 *                infinite one is dropped without counting.  Overwritten, never accumulated; nothing outside the n entries is written.  count may be NULL.
 *   memory       flags 0: rays, rgb_sum and count are host memory, staged through buffers of the context that only grow; TGHIP_DEVELOP_DEVICE_POINTERS:
 *                memory of the context's device, rays 16-byte aligned, rgb_sum and count 4-byte aligned -- nothing is allocated per call once the
 *                scratch (the virtual image's framebuffer, its tile seeds, the pool) has grown.  Returns when the answers are complete.
 *   context      runs on the context's stream and waits for a running pass like tghip_develop; leaves the framebuffer (internal or bound), the
 *                SampleRecords, the auxiliary buffers, the per-sample buffer and with them a resumed render exactly as they were: the passes after a
 *                query are bit for bit the passes without it.  "max_slots", "max_items", "chunk_samples" and the other options are honoured and never
 *                change an answer ("chunk_samples" is accepted and does not size a query's items: the order of the additions is part of the answer); the
 *                counters advance as by a pass.
 * A ray with a non-finite component or a zero direction gets an unspecified answer; the call returns.  Directions are expected to have unit length, as
 * the camera's have.  n == 0 succeeds.  TGHIP_E_NOSCENE without an upload.  TGHIP_E_INVALID, the context still usable (tghip_last_error says which): no
 * description, NULL rays or rgb_sum with n > 0, unknown flag bits, non-zero reserved words, spp_end <= spp_begin, TGHIP_RADIANCE_SOBOL on a scene without
 * sobol_matrices, n > 2^31 - 1, misaligned device pointers.  TGHIP_E_UNSUPPORTED: n (spp_end - spp_begin) >= 2^32 samples, the size at which the pass
 * plan refuses a record pass (tungsten_host.h: tgh_query_radiance_check is the same check on its own). */
#define TGHIP_RADIANCE_SOBOL 2u      /* flags; bit 0 stays TGHIP_DEVELOP_DEVICE_POINTERS */
typedef struct TgHipRadianceQueryDesc {
    uint32_t flags;                  /* TGHIP_DEVELOP_DEVICE_POINTERS | TGHIP_RADIANCE_SOBOL */
    uint32_t seed;
    uint32_t spp_begin, spp_end;     /* sample indices [spp_begin, spp_end) of every ray */
    uint32_t sobol_seed;             /* TGHIP_RADIANCE_SOBOL: the SobolPathSampler seed every ray's "tile" has */
    uint32_t reserved[3];            /* zero */
} TgHipRadianceQueryDesc;            /* 32 B */
int tghip_query_radiance(tghip_ctx *ctx, const TgHipRadianceQueryDesc *desc, const TgHipRay *rays, float *rgb_sum /* n*3 */, uint32_t *count /* n, may be NULL */,
                         size_t n);
/* Instrumentation: HIP-event time of the launches of the context's last tghip_query_radiance -- the pass and the copy of its answers --, in
 * milliseconds (profiles/radiance_query/bench.txt) */
int tghip_query_radiance_kernel_time(tghip_ctx *ctx, double *ms);
/* What is at the closest hit of caller-supplied rays: position, geometric and shading normal, texture coordinates, primitive, instance and material, the
 * material's albedo and the emitted radiance -- the question between tghip_query_rays (where) and tghip_query_radiance (what arrives).  Two launches
 * on the context's stream (csrc/hip/surface_query.hip): tghip_query_rays' closest-hit walk, which keeps the hit and the instance it was reached
 * through in scratch of the context, and a dense launch, one lane per ray, that describes the hit and writes the answer.
 *   the hit      rec and t are bit for bit what tghip_query_rays (TGHIP_QUERY_CLOSEST) returns for the same ray on the same context, in every kind of
 *                scene and at the edge of [tmin, tmax) alike: the walk is that call's.
 *   its fields   ng, ns, uv: IntersectionInfo::Ng, ::Ns, ::uv of the primitive (Primitive::intersectionInfo; through an instance the normals rotated to
 *                world space, primitives/Instance.cpp:337-346) -- the primitive's own values, the ones the normal output buffer records: nothing is
 *                flipped for two-sided shading, no bump map is applied.  p = ray.o + ray.d*t in float32, unfused (TraceableScene.hpp:184), for an
 *                instanced hit too.  albedo = (*bsdf->albedo())[info] as PathTracer.cpp:83-88 takes it: a `transparency` material gives its base's.
 *                emission = Primitive::evalDirect at the hit when the primitive is emissive (zero from its back side), else zero.  object: the
 *                primitive, for an instanced hit the `instances` object; bsdf: the global index of the hit's material; instance: the record index of
 *                the TGHIP_REC_INSTANCE record the hit was reached through, -1 = none.
 *   a miss       rec, instance, object and bsdf are -1 and every other word is zero -- unless TraceableScene::intersectInfinites
 *                (TraceableScene.hpp:194-209) finds an emitter along d (the last infinite light wins; a cap only inside its angle): then flags =
 *                TGHIP_SURFACE_INFINITE, object is the emitter, uv its direction's (0, 0 for a cap) and emission its texture there.
 *   arithmetic   one instantiation under the all-features family's mask (every record kind and texture type, the reference's tie rule on a cube's
 *                edges): an answer never depends on which shading family the scene's passes use.
 *   memory       flags 0: rays and out are host memory, staged through buffers of the context that only grow; TGHIP_DEVELOP_DEVICE_POINTERS: both are
 *                memory of the context's device, 16-byte aligned.  Nothing is allocated per call once the scratch has grown.
 * Runs on the context's stream, waits for a running pass like tghip_query_rays, returns when the answers are complete and leaves the framebuffer, the
 * SampleRecords, the auxiliary and the per-sample buffers as they were.  "query_blocks" and "query_refill_at" steer the walk as they steer
 * tghip_query_rays' and never change an answer.  A ray with a non-finite component or a zero direction gets an unspecified answer; the call returns.
 * n == 0 succeeds.  TGHIP_E_NOSCENE without an upload.  TGHIP_E_INVALID, the context still usable (tghip_last_error says which): no description, NULL
 * rays or out with n > 0, unknown flag bits, non-zero reserved words, n > 2^31 - 1, misaligned device pointers (tungsten_host.h:
 * tgh_query_surface_check is the same check on its own). */
#define TGHIP_SURFACE_HIT       1u   /* a finite primitive was hit: every field below is filled */
#define TGHIP_SURFACE_BACK_SIDE 2u   /* IntersectionTemporary's back-side answer of the primitive (Info::backSide) */
#define TGHIP_SURFACE_EMISSIVE  4u   /* the primitive hit has an emission (Primitive::isEmissive) */
#define TGHIP_SURFACE_INFINITE  8u   /* no hit; an infinite emitter lies along the ray: object, uv, emission are its */
typedef struct TgHipSurface {
    float p[3];   float t;           /* ray.o + ray.d*t (TraceableScene.hpp:184), float32, unfused */
    float ng[3];  int32_t rec;       /* IntersectionInfo::Ng; the record, as TgHipHit::rec */
    float ns[3];  int32_t instance;  /* IntersectionInfo::Ns; record index of the TGHIP_REC_INSTANCE record the hit was reached through, -1 = none */
    float uv[2];  int32_t object, bsdf;   /* IntersectionInfo::uv; the primitive (for an instanced hit the `instances` object); global bsdf index */
    float albedo[3];   uint32_t flags;
    float emission[3]; uint32_t reserved; /* 0 */
} TgHipSurface;                      /* 96 B */
typedef struct TgHipSurfaceQueryDesc { uint32_t flags, reserved[3]; } TgHipSurfaceQueryDesc;   /* flags: TGHIP_DEVELOP_DEVICE_POINTERS */
int tghip_query_surface(tghip_ctx *ctx, const TgHipSurfaceQueryDesc *desc, const TgHipRay *rays, TgHipSurface *out, size_t n);
/* Instrumentation: HIP-event time of the two launches of the context's last tghip_query_surface, in milliseconds; with the option
 * "surface_time_stage" = 1 that of its dense launch alone (profiles/surface_query/bench.txt).  The option changes no answer. */
int tghip_query_surface_kernel_time(tghip_ctx *ctx, double *ms);
/* How much light gets along caller-supplied rays: TraceBase::generalizedShadowRay (integrators/TraceBase.cpp:62-133, generalizedShadowRayImpl<false>) on
 * the segment [tmin, tmax) of every ray -- the visibility the path tracer's own shadow rays see: `forward` boundaries and `transparency` cut-outs let light
 * through, participating media attenuate it, the primitive the rays are aimed at is left out.  (TGHIP_QUERY_OCCLUDED is geometry only.)  A small wavefront
 * of its own on the context's stream (csrc/hip/transmittance_query.hip): per round a closest-hit walk -- tghip_query_rays' -- over the rays still under
 * way, and a dense launch, one lane per such ray, that does the rest of the round and either writes the ray's answer or hands it to the next round.
 *   closest hit  every round takes the closest hit of the current segment: bit for bit what tghip_query_rays (TGHIP_QUERY_CLOSEST) answers for the segment's
 *                (o, d, tmin, tmax) on the same context, in every kind of scene.  Infinite emitters are never hit.
 *   a hit that   the material has no TGHIP_LOBE_FORWARD: rgb = 0.  Otherwise transparency = bsdf->eval(forward event) (the frame flipped for two-sided
 *   is not the   shading exactly as the path tracer's shadow walk flips it, all-features arithmetic); transparency == 0: rgb = 0; throughput *= transparency,
 *   end cap      bounce++, and bounce >= max_bounces: rgb = 0.
 *   medium       then, if the ray is in a medium: throughput *= transmittance(the ray up to the hit, or up to tmax on a miss; startsOnSurface;
 *                endsOnSurface) -- AFTER the transparency, the reference's order (:97, 104-112), and with the caller's endsOnSurface for EVERY
 *                segment (:111), not the constant `true` of a pass's shadow rays.
 *   the end      on a miss, or when the hit is the end cap: rgb = throughput if bounce >= min_bounces, else 0.  A quad end cap is only found when
 *                Embree's slab test lets the ray into its flat box: culled, the walk ends as at the end cap but the segment's medium length is tmax.
 *   otherwise    medium = selectMedium(hit primitive, medium, !backSide), startsOnSurface = true, o = o + d*t (float32, unfused), remaining -= t,
 *                tmin = 5e-4, tmax = remaining, and the next round.
 *   crossed      the number of times `bounce++` above ran, whatever ended the walk.
 *   media        NULL: every ray starts in desc->medium; else n words, ray i starts in media[i] (an index in TgHipSceneDesc::media, TGHIP_MEDIUM_NONE or
 *                TGHIP_MEDIUM_OF_CAMERA) and desc->medium is only checked.
 *   memory       flags without TGHIP_DEVELOP_DEVICE_POINTERS: rays, media and out are host memory, staged through buffers of the context that only
 *                grow; with it: memory of the context's device, rays and out 16-byte aligned, media 4-byte aligned.  Nothing is allocated per call
 *                once the scratch has grown.
 * The pdfs (generalizedShadowRayAndPdfs), the emission at the end cap with a mesh light's distance test (attenuatedEmission) and per-ray end caps are not
 * part of the call (tghip_query_direct below has the latter two).  Runs on the context's stream, waits for a running pass like tghip_query_rays, returns when the answers are complete and leaves the
 * framebuffer, the SampleRecords, the auxiliary and the per-sample buffers as they were.  "query_blocks" and "query_refill_at" steer the walk and never
 * change an answer.  A per-ray media[i] out of range, a non-finite ray component or a zero direction gives that ray an unspecified answer; the call
 * returns.  n == 0 succeeds.  TGHIP_E_NOSCENE without an upload -- decided before the arguments are looked at, a missing description apart: the check
 * reads the uploaded scene's tables, so on a context without a scene a malformed call answers TGHIP_E_NOSCENE too (its siblings, whose checks need
 * no scene, answer TGHIP_E_INVALID there).  TGHIP_E_INVALID, the context still usable (tghip_last_error says which): no description,
 * NULL rays or out with n > 0, unknown flag bits, non-zero reserved words, n > 2^31 - 1, misaligned device pointers, desc->medium below -2 or >=
 * num_media or naming an operand entry of an `interpolated` medium (tghip_debug_medium's rule), end_cap outside the objects or naming an `instances`
 * object or an infinite emitter, bounce > 255 (tungsten_host.h: tgh_query_transmittance_check is the same check on its own). */
#define TGHIP_TRANSMITTANCE_STARTS_ON_SURFACE 2u   /* flags; bit 0 stays TGHIP_DEVELOP_DEVICE_POINTERS */
#define TGHIP_TRANSMITTANCE_ENDS_ON_SURFACE   4u
#define TGHIP_MEDIUM_NONE      (-1)
#define TGHIP_MEDIUM_OF_CAMERA (-2)                /* the medium the scene's camera is in, as tghip_query_radiance starts */
typedef struct TgHipTransmittanceQueryDesc {
    uint32_t flags;
    int32_t  medium;      /* medium every ray starts in when `media` is NULL: index in TgHipSceneDesc::media, or one of the two above */
    int32_t  end_cap;     /* object index of the primitive the rays are aimed at (generalizedShadowRay's endCap), -1 = none */
    uint32_t bounce;      /* the bounce count the walk starts with */
    uint32_t reserved[4]; /* zero */
} TgHipTransmittanceQueryDesc;                     /* 32 B */
typedef struct TgHipTransmittance { float rgb[3]; uint32_t crossed; } TgHipTransmittance;   /* 16 B */
int tghip_query_transmittance(tghip_ctx *ctx, const TgHipTransmittanceQueryDesc *desc, const TgHipRay *rays,
                              const int32_t *media /* n start media, may be NULL */, TgHipTransmittance *out, size_t n);
/* Instrumentation: HIP-event time from the first launch to the last of the context's last tghip_query_transmittance, in milliseconds -- every round's two
 * launches and the one-word read-backs between the rounds (profiles/transmittance_query/bench.txt) */
int tghip_query_transmittance_kernel_time(tghip_ctx *ctx, double *ms);
/* ... and the rounds that call ran: 1 + the most surfaces a ray of the batch went on behind, 1 in a scene without a forward-lobe BSDF */
int tghip_query_transmittance_rounds(tghip_ctx *ctx, uint32_t *rounds);
/* How much light the scene's emitters send DIRECTLY to the closest hit of caller-supplied rays -- or to their origins inside a medium: the path tracer's
 * next-event estimation, TraceBase::estimateDirect (integrators/TraceBase.cpp:483-494) and volumeEstimateDirect (:470-481), sample by sample.  A small
 * wavefront of its own on the context's stream (csrc/hip/direct_query.hip): the closest-hit walk of tghip_query_surface, a dense launch, one lane per
 * (ray, sample), that draws the samples and decides what needs no walk, rounds of tghip_query_transmittance's walk over the shadow rays still under way
 * with a dense launch each, and a launch that adds every ray's samples up.
 *   surface      (no TGHIP_DIRECT_VOLUME)  the point is the closest hit of ray i in [tmin, tmax): bit for bit tghip_query_surface's on the same context;
 *   mode         `rec` is its TgHipHit::rec.  A miss answers zeros with rec = -1 and count = 0.  At a hit every sample s is one
 *                estimateDirect(event, medium, desc->bounce, ray, &transmittance), event = makeLocalScatterEvent(data, info, ray, sampler)
 *                (TraceBase.cpp:24-51: the frame flipped for two-sided shading), medium the one the ray travels in, transmittance initialised to -1
 *                as PathTracer.cpp:70 does.  Inside, operation for operation: chooseLight; sampleDirect's early return for pure-specular and forward
 *                materials; lightSample and -- not for a Dirac light -- bsdfSample (:246-321) with isConsistent, selectMedium by the geometric side of
 *                each shadow ray, attenuatedEmission (:144-174: the light's own intersect, the 1 + 1e-3 distance test, a Dirac light's ray cut at the
 *                sampled distance, generalizedShadowRay with the light as end cap, startsOnSurface = endsOnSurface = true), evalDirect, directPdf and
 *                the power heuristic.  A triangle-mesh emitter's own intersect is the scene walk, as in a pass: its hit is the first one of the shadow
 *                walk that is the mesh.
 *   volume mode  (TGHIP_DIRECT_VOLUME)  the point is rays[i].o, rays[i].d the direction the path arrived along (parentRay.dir()); tmin and tmax are
 *                ignored and no walk precedes the estimate.  Every sample is one volumeEstimateDirect (:470-481, 323-381, 402-414) with the phase
 *                function of the start medium: shadow rays with epsilon 0, startsOnSurface = false, no selectMedium.  A ray that starts in no medium
 *                answers zeros with count = 0.  rec = -1, and visibility_count stays 0: the reference passes no `transmittance` there.
 *   rgb          the float32 sum of the samples' estimates, added one by one in sample-index order from zero.  Multiplied by no throughput; nothing is
 *                added for an emissive hit.  The conditions around the call in handleSurface (enable_light_sampling, bounce < max_bounces - 1) are
 *                the caller's business; min_bounces and max_bounces act only where generalizedShadowRay reads them.  A scene without lights answers
 *                zeros.  No option and no internal division of the work changes a bit of it.
 *   visibility   the sum, in the same order, of transmittance.avg() over the samples whose light sample got as far as its shadow ray, and
 *   .._count     how many those were: what PathTracer.cpp:93-94 feeds the visibility output with.
 *   count        the samples taken: spp_end - spp_begin at a hit (in a medium), 0 otherwise.
 *   numbers      ray i, sample s draws from the counter-based stream keyed (seed, i, s) (csrc/hip/pt_math.h: rngStart), s in [spp_begin, spp_end); after
 *                `skip` numbers drawn and thrown away, in the reference's order: chooseLight's one number when it is called (light = -1) and the
 *                scene has more than one light, then sampleDirect's, then the BSDF's or the phase function's.  There is no Sobol' form.
 *   light        -1: chooseLight.  k >= 0: the light in slot k of TgHipSceneDesc::lights with weight 1 and no chooseLight draw.
 *   medium,      as tghip_query_transmittance's: media NULL, every ray starts in desc->medium; else n words, ray i starts in media[i] and desc->medium
 *   media        is only checked.
 *   memory       flags without TGHIP_DEVELOP_DEVICE_POINTERS: rays, media and out are host memory, staged through buffers of the context that only
 *                grow; with it: memory of the context's device, rays and out 16-byte aligned, media 4-byte aligned.  Nothing is allocated per call
 *                once the scratch has grown (it grows to a fixed number of items; larger calls run in parts).
 * All-features arithmetic, so an answer never depends on the scene's shading family.  Runs on the context's stream, waits for a running pass like
 * tghip_query_rays, returns when the answers are complete and leaves the framebuffer, the SampleRecords, the auxiliary and the per-sample buffers as
 * they were.  "query_blocks" and "query_refill_at" steer the walks and never change an answer.  n == 0 succeeds.  TGHIP_E_NOSCENE without an upload,
 * decided before the arguments are looked at, a missing description apart, as tghip_query_transmittance.  TGHIP_E_INVALID, the context still usable:
 * no description, NULL rays or out with n > 0, unknown flag bits, n > 2^31 - 1, misaligned device pointers, desc->medium below -2 or >= num_media or
 * naming an operand entry of an `interpolated` medium, spp_end <= spp_begin, skip > 1024, light below -1 or >= num_lights, bounce > 255, volume mode
 * with media == NULL and a desc->medium that resolves to no medium.  TGHIP_E_UNSUPPORTED: n (spp_end - spp_begin) >= 2^32 (tungsten_host.h:
 * tgh_query_direct_check is the same check on its own). */
#define TGHIP_DIRECT_VOLUME 2u           /* flags; bit 0 stays TGHIP_DEVELOP_DEVICE_POINTERS */
typedef struct TgHipDirectQueryDesc {
    uint32_t flags;
    uint32_t seed;
    uint32_t spp_begin, spp_end;         /* sample indices [spp_begin, spp_end) of every ray */
    int32_t  medium;                     /* as TgHipTransmittanceQueryDesc::medium: index, TGHIP_MEDIUM_NONE, TGHIP_MEDIUM_OF_CAMERA */
    uint32_t bounce;                     /* the `bounce` handed to estimateDirect (a pass's camera vertex hands 1) */
    int32_t  light;                      /* -1: chooseLight; k >= 0: slot k of TgHipSceneDesc::lights, weight 1, no chooseLight draw */
    uint32_t skip;                       /* numbers of the stream drawn and thrown away first, <= 1024 */
} TgHipDirectQueryDesc;                  /* 32 B */
typedef struct TgHipDirect {
    float    rgb[3];                     /* float32 sum of the samples' estimates, added one by one in sample-index order from zero */
    float    visibility;                 /* sum of transmittance.avg() over the samples that recorded one */
    uint32_t count, visibility_count;
    int32_t  rec;                        /* surface mode: TgHipHit::rec of the hit, -1 = miss; volume mode: -1 */
    uint32_t reserved;                   /* 0 */
} TgHipDirect;                           /* 32 B */
int tghip_query_direct(tghip_ctx *ctx, const TgHipDirectQueryDesc *desc, const TgHipRay *rays,
                       const int32_t *media /* n start media, may be NULL */, TgHipDirect *out, size_t n);
/* Instrumentation: HIP-event time from the first launch to the last of the context's last tghip_query_direct, in milliseconds -- the walks, the dense
 * launches and the one-word read-backs between the rounds (profiles/direct_query/bench.txt) */
int tghip_query_direct_kernel_time(tghip_ctx *ctx, double *ms);
/* Paths whose state the CALLER holds, advanced vertex by vertex: one call runs `turns` turns of PathTracer::traceSample's loop
 * (integrators/path_tracer/PathTracer.cpp:50-131) on n states -- TraceBase::handleSurface (integrators/TraceBase.cpp:516-568), handleVolume (:496-514),
 * Medium::sampleDistance, the roulette, the NaN guards and handleInfiniteLights (:570-578).  Chained until no path is alive it returns
 * tghip_query_radiance's answer bit for bit; in between the caller may look at the throughput, end a path by its own rule, hand in a direction of
 * its own, reorder, drop or split the batch: a turn is a pure function of (state, uploaded scene and its integrator settings), and a TgHipPath is the
 * whole state.  A small wavefront of its own on the context's stream (csrc/hip/vertex_query.hip): the closest-hit walk of tghip_query_surface over the
 * live paths' rays, a dense front stage, the shadow walks and rounds of tghip_query_direct, a dense back stage.
 *   start        TGHIP_VERTEX_START: state i is made from rays[i] first -- throughput 1, emission 0, bounce 0, wasSpecular, medium media[i] (or
 *                desc->medium where media is NULL), the medium's state reset, the stream rngStart(seed, first_index + i, sample) behind first_number
 *                numbers (csrc/hip/pt_math.h).  first_number = 2 makes a pinhole camera's own rays give that camera's samples, as
 *                tghip_query_radiance does.  `paths` is then written only.  Without the flag rays and media must be NULL and `paths` is read.
 *   one turn     of a live path (status 0), operation for operation in the reference's order: the closest hit in [tmin, tmax) -- rec and t are bit for
 *                bit tghip_query_rays' (TGHIP_QUERY_CLOSEST) on the same context, a hit counting when t < tmax; with no hit and no medium the
 *                epilogue (:128-131: handleInfiniteLights under min_bounces <= bounce < max_bounces, the NaN guard, ESCAPED); otherwise
 *                sampleDistance, and at a surface makeLocalScatterEvent and handleSurface with estimateDirect exactly as tghip_query_direct
 *                computes it (bounce + 1, the path's medium, the path's stream), in a medium handleVolume with volumeEstimateDirect.
 *                emission += estimateDirect*throughput comes before the emissive hit's term (TraceBase.cpp:537-543), the roulette (:111-117) draws
 *                after the BSDF, the NaN guards (:119-122) read the emission after both additions.  The next ray is ray.scatter(hitpoint, wo,
 *                epsilon) at a surface and (p, w, 0) in a medium, tmax infinite, the medium selected by the geometric side and its state reset at a
 *                surface.  bounce++; at max_bounces the path ends in this turn, so a path never costs a walk the reference would not make.
 *   turns        the call runs desc->turns turns, or stops earlier when no path is alive.  *alive: the paths still alive afterwards.
 *   ended paths  a path that is not alive comes back byte for byte as it came in.
 *   bad states   a state whose medium is out of range or whose ray has a non-finite component or a zero direction gets an unspecified answer; the
 *                call returns and nothing outside the n states is written.
 *   memory       flags without TGHIP_DEVELOP_DEVICE_POINTERS: rays, media, paths and alive are host memory, staged through buffers of the context
 *                that only grow; with it: memory of the context's device, rays and paths 16-byte aligned, media and alive 4-byte aligned (alive,
 *                one word copied once the turns are through, may be a word of host memory even then).  The
 *                scratch grows to a fixed number of paths; larger calls run in parts, which changes no bit.
 * All-features arithmetic and the keyed PCG stream only (no Sobol' form), as tghip_query_direct.  MediumState's mediumBounces is NOT part of the state:
 * TgHipSettings::low_order_scattering and include_surfaces keep their defaults in every scene this library uploads, so nothing reads it.  Runs on the
 * context's stream, waits for a running pass like tghip_query_rays, returns when the states are complete and leaves the framebuffer, the SampleRecords,
 * the auxiliary and the per-sample buffers as they were.  "query_blocks" and "query_refill_at" steer the walks and never change an answer.  n == 0
 * succeeds.  TGHIP_E_NOSCENE without an upload, decided as tghip_query_transmittance decides it.  TGHIP_E_INVALID, the context still usable: no
 * description, NULL paths with n > 0, TGHIP_VERTEX_START without rays, rays or media without it, unknown flag bits, a non-zero reserved word,
 * turns == 0, first_number > 1024, n > 2^31 - 1, misaligned device pointers, desc->medium below -2 or >= num_media or naming an operand entry of an
 * `interpolated` medium (tungsten_host.h: tgh_query_vertex_check is the same check on its own). */
#define TGHIP_VERTEX_START 2u            /* flags; bit 0 stays TGHIP_DEVELOP_DEVICE_POINTERS */
typedef struct TgHipVertexQueryDesc {
    uint32_t flags;
    uint32_t seed;
    uint32_t sample;                     /* the sample index of the stream's key */
    uint32_t first_index;                /* ray i is keyed first_index + i */
    uint32_t first_number;               /* numbers of the stream drawn and thrown away first, <= 1024 */
    int32_t  medium;                     /* as TgHipTransmittanceQueryDesc::medium: index, TGHIP_MEDIUM_NONE, TGHIP_MEDIUM_OF_CAMERA */
    uint32_t turns;                      /* >= 1 */
    uint32_t reserved;                   /* 0 */
} TgHipVertexQueryDesc;                  /* 32 B */
/* TgHipPath::status: 0 = alive, else why the path ended */
enum { TGHIP_PATH_ALIVE = 0,
       TGHIP_PATH_END_ESCAPED = 1,          /* the loop's condition failed, or PathTracer.cpp:59-60: the epilogue ran */
       TGHIP_PATH_END_MAX_BOUNCES = 2,      /* bounce reached max_bounces in this turn */
       TGHIP_PATH_END_ABSORBED = 3,         /* sampleDistance, bsdf.sample, isConsistent or the phase sample failed (:54-55, 98-99, 103-105) */
       TGHIP_PATH_END_ZERO_THROUGHPUT = 4,  /* :108-109, then the epilogue */
       TGHIP_PATH_END_ROULETTE = 5,         /* :116 */
       TGHIP_PATH_END_NAN = 6 };            /* :119-122, 130-131: the emission is zero, as the reference returns its NaN colours */
#define TGHIP_PATH_WAS_SPECULAR 1u       /* TgHipPath::flags */
typedef struct TgHipPath {
    float    o[3], tmin, d[3], tmax;     /* the ray the next turn traces: laid out as a TgHipRay */
    float    throughput[3];
    float    emission[3];                /* what traceSample would return if the path ended now */
    uint32_t status;                     /* TGHIP_PATH_ALIVE or a TGHIP_PATH_END_* */
    int32_t  medium;                     /* the medium the ray travels in: an index in TgHipSceneDesc::media, or -1 */
    uint32_t medium_state_bounce;        /* MediumState::bounce; firstScatter is medium_state_bounce == 0, as in TgHipMediumCase */
    uint32_t bounce;
    uint32_t flags;                      /* TGHIP_PATH_WAS_SPECULAR */
    int32_t  rec;                        /* TgHipHit::rec of the last turn's walk, -1 = miss */
    float    t;                          /* ... and its distance, 0 on a miss */
    uint32_t rng_state[2];               /* the PCG state, low word first */
    uint32_t key;                        /* the index the stream's increment is made of */
    uint32_t drawn;                      /* numbers taken from the stream so far, first_number included */
    uint32_t reserved[3];                /* carried along unchanged; TGHIP_VERTEX_START writes zeros */
} TgHipPath;                             /* 112 B: seven 16-byte vectors */
int tghip_query_vertex(tghip_ctx *ctx, const TgHipVertexQueryDesc *desc, const TgHipRay *rays /* TGHIP_VERTEX_START only: n rays */,
                       const int32_t *media /* TGHIP_VERTEX_START only: n start media, may be NULL */,
                       TgHipPath *paths /* n states: read and written; with START written only */, size_t n,
                       uint32_t *alive /* paths still alive afterwards, may be NULL */);
/* Instrumentation: HIP-event time from the first launch to the last of the context's last tghip_query_vertex, in milliseconds -- the walks, the dense
 * launches and the one-word read-backs between them (profiles/vertex_query/bench.txt) */
int tghip_query_vertex_kernel_time(tghip_ctx *ctx, double *ms);
/* Self-test of the device's libm restatements (csrc/hip/pt_libm.h: glibc's sinf / cosf / logf / expf / atan2f / powf / cbrtf as the shading
 * kernels call them, pt_math.h: acosf): y[i] = fn(x[i]) evaluated ON THE DEVICE, host pointers.  fn: TGHIP_LIBM_*.  The two-argument
 * functions read their operands interleaved from x (2 n floats): ATAN2F y[i] = atan2f(x[2i], x[2i+1]), POWF y[i] = powf(x[2i], x[2i+1]).
 * EMBREE_RCP / RCPPS: Embree's rcp(a) = r*(2 - r*a) and its r = Intel's RCPPS estimate as the triangle test restates them (pt_scene.h: embreeRcp,
 * rcppsIntel).  The GPU tests compare y with the host libm / the oracle's restatement bit for bit. */
enum { TGHIP_LIBM_SINF = 0, TGHIP_LIBM_COSF = 1, TGHIP_LIBM_LOGF = 2, TGHIP_LIBM_EXPF = 3, TGHIP_LIBM_SINCOS_SIN = 4, TGHIP_LIBM_SINCOS_COS = 5,
       TGHIP_LIBM_ACOSF = 6, TGHIP_LIBM_ATAN2F = 7, TGHIP_LIBM_POWF = 8, TGHIP_LIBM_CBRTF = 9,
       TGHIP_LIBM_EMBREE_RCP = 10, TGHIP_LIBM_RCPPS = 11, TGHIP_LIBM_TANF = 12,
       /* double precision (AtmosphericMedium::inverseOpticalDepth: std::exp / log / erf / sqrt on doubles): x and y then point to n DOUBLES */
       TGHIP_LIBM_EXPD = 13, TGHIP_LIBM_LOGD = 14, TGHIP_LIBM_ERFD = 15, TGHIP_LIBM_SQRTD = 16,
       /* float again: glibc's sinhf on its restated domain (0, 10] (the rough_wire BCSDF's sinh(1/v), v >= 0.1), NaN outside it */
       TGHIP_LIBM_SINHF = 17 };
int tghip_debug_libm(tghip_ctx *ctx, int fn, const float *x, float *y, size_t n);
/* Self-test of the device's BSDF code (csrc/hip/pt_scene.h: bsdfEval / bsdfPdf / bsdfSample, the wrappers the shading kernels call) on caller-supplied
 * cases against the uploaded scene's flattened bsdf table, one thread per case (csrc/hip/debug_units.hip), host pointers.  Per case: eval and pdf of
 * (wi, wo), then sample(wi) drawing from the counter-based stream started as a path's is with (seed, stream, 0), then ONE further number of that
 * stream -- so the caller, who can produce the same stream, sees how many numbers the sample consumed.  `variant` selects the instantiation: the
 * BSDF type / feature mask of one shading family (csrc/hip/pt_wavefront.h), each without the Sobol' sampler.  A type outside the variant's mask folds
 * away exactly as in that family's shading kernel (black eval, zero pdf, failed sample).  Outputs of a failed sample are unspecified.
 * TGHIP_E_INVALID (context left usable) for null pointers with n > 0, a bsdf index outside the table, an unknown variant, or no scene; n == 0 succeeds. */
enum { TGHIP_BSDF_VARIANT_LEAN = 0, TGHIP_BSDF_VARIANT_SIMPLE = 1, TGHIP_BSDF_VARIANT_COAT = 2, TGHIP_BSDF_VARIANT_GLASS = 3,
       TGHIP_BSDF_VARIANT_PLASTIC = 4, TGHIP_BSDF_VARIANT_MEDIA = 5, TGHIP_BSDF_VARIANT_TAIL = 6, TGHIP_BSDF_VARIANT_FULL = 7,
       TGHIP_BSDF_VARIANT_ALL = 8, TGHIP_BSDF_VARIANT_COUNT = 9 };
typedef struct TgHipBsdfCase {
    int32_t  bsdf;            /* index in the flattened table (TgHipSceneDesc::bsdfs) */
    uint32_t requested;       /* TGHIP_LOBE_* set */
    float    wi[3], wo[3];    /* local directions (shading normal = +z) */
    float    uv[2];
    uint32_t seed, stream;    /* the sampler: rngStart(seed, stream, 0) */
    uint32_t variant;         /* TGHIP_BSDF_VARIANT_* */
    uint32_t reserved;
} TgHipBsdfCase;
typedef struct TgHipBsdfResult {
    float    f[3], pdf;                       /* eval, pdf */
    uint32_t sample_ok;
    float    sample_wo[3], sample_weight[3], sample_pdf;
    uint32_t sampled;                         /* the sampled lobe */
    float    next;                            /* the stream's next number after the sample returned */
    uint32_t reserved[2];
} TgHipBsdfResult;
int tghip_debug_bsdf(tghip_ctx *ctx, const TgHipBsdfCase *cases, TgHipBsdfResult *results, size_t n);
/* What the shading-class rule sees of the uploaded scene's bsdfs (num_bsdfs entries each; any pointer may be NULL): type_mask = the set of bsdf types
 * inside the material, nested ones included (bit = 1 << TGHIP_BSDF_*; bit 19 when a microfacet bsdf inside uses the Phong distribution; bit 24 when a
 * texture inside is a bitmap; bits 20 - 23 together when the scene holds a `disk` or `blade` texture anywhere -- such a scene is shaded by the all-features
 * family throughout, so TGHIP_BSDF_VARIANT_ALL alone covers its entries; the same four bits when the scene holds a fibre BCSDF, TGHIP_BSDF_LAMBERTIAN_FIBER / _ROUGH_WIRE, anywhere:
 * those two types have no bit of their own, bits 19 and 20 being the Phong and the bump feature), forward = 1 when it has a forward lobe, covered = 1 when family `variant` is allowed to shade it by the rule that sorts
 * materials into shading classes and picks each class's kernel.  variant_mask (one word): the type / feature mask the variant's kernel is compiled for. */
int tghip_debug_bsdf_info(tghip_ctx *ctx, int variant, uint32_t *type_mask, uint32_t *forward, uint32_t *covered, uint32_t *variant_mask);
/* Self-test of the device's light code (csrc/hip/pt_scene.h: chooseLight / lightSampleDirect / lightApproximateRadiance / lightIntersect / lightEvalDirect /
 * lightDirectPdf) on caller-supplied cases against the uploaded scene, one thread per case (csrc/hip/debug_units.hip), host pointers; the calls are made
 * as the shading kernels' next-event estimation makes them, under the feature mask of family `variant` (no Sobol' sampler).  Per case:
 *   choose   chooseLight(p) drawing from the stream (seed, stream, 0): the chosen OBJECT index (-1: none), its weight, and the stream's next number;
 *   sample   lightSampleDirect of the light in slot `light` from p, drawing from the stream (seed, stream, 1): ok, d, dist, pdf, the stream's next number;
 *   approx   lightApproximateRadiance of that light at p;
 *   hit      lightIntersect with the ray (p, w, tmin 5e-4, tmax inf): hit, t, u, v, back_side and, where it hits, lightEvalDirect and lightDirectPdf.
 * A mesh emitter is never intersected here (its hit leg belongs to the shadow kernel): hit = 0.  Neither is a point light, whose shadow ray ends at the
 * sampled distance: hit = 0, and direct_pdf is lightDirectPdf with the hit record the shading kernel builds there (t = the sampled dist).
 * Outputs behind a failed choose / sample / intersect are unspecified.  TGHIP_E_INVALID (context left usable) for null pointers with n > 0, a light slot
 * outside TgHipSceneDesc::lights, an unknown variant, or no scene; n == 0 succeeds. */
typedef struct TgHipLightCase {
    int32_t  light;           /* slot in TgHipSceneDesc::lights */
    uint32_t variant;         /* TGHIP_BSDF_VARIANT_* */
    float    p[3], w[3];      /* the shading point; a unit direction */
    uint32_t seed, stream;    /* the samplers: rngStart(seed, stream, 0) and (seed, stream, 1) */
} TgHipLightCase;             /* 40 B */
typedef struct TgHipLightResult {
    int32_t  chosen;          /* object index of the chosen light, -1 = none */
    float    choose_weight;
    uint32_t sample_ok;
    float    d[3], dist, pdf;
    float    approx;
    uint32_t hit;
    float    t, u, v;
    uint32_t back_side;
    float    emission[3], direct_pdf;
    float    choose_next, sample_next;   /* the two streams' next numbers after the calls returned */
    uint32_t reserved[4];
} TgHipLightResult;           /* 96 B */
int tghip_debug_light(tghip_ctx *ctx, const TgHipLightCase *cases, TgHipLightResult *results, size_t n);
/* What the light code of family `variant` needs of the uploaded scene's sampled lights (num_lights entries each; any pointer may be NULL): needs = the
 * feature bits the branches of the light's emitter type sit behind in csrc/hip/pt_scene.h and the shading kernels (csrc/host/SceneCheck.cpp: lightNeeds;
 * the bits are those of csrc/hip/pt_variants.h: FEAT_SOLIDS, FEAT_INFINITE, FEAT_BITMAP, FEAT_MESHLIGHT, FEAT_CYLINDER, the four bits of FEAT_FAMILY_ALL
 * together, FEAT_MULTILIGHT), covered = 1 when the variant's mask holds them all.  variant_mask (one word): the mask the variant's kernel is compiled for. */
int tghip_debug_light_info(tghip_ctx *ctx, int variant, uint32_t *needs, uint32_t *covered, uint32_t *variant_mask);
/* Self-test of the device's medium code (csrc/hip/pt_scene.h: mediumSampleDistance / mediumTransmittance / phaseEval / phaseSample) on caller-supplied
 * cases against the uploaded scene's media, one thread per case (csrc/hip/debug_units.hip), host pointers; the calls are made as k_shade and the shadow
 * walks make them, under the feature mask of family `variant` (no Sobol' sampler) -- which must be one that carries the media code (FEAT_MEDIA:
 * tghip_debug_bsdf_info's variant_mask says which; today TGHIP_BSDF_VARIANT_MEDIA and TGHIP_BSDF_VARIANT_ALL).  Per case:
 *   distance  mediumSampleDistance along the ray (p, d) up to max_t (+inf: the segment left the scene) with the medium's bounce count state_bounce
 *             (firstScatter = state_bounce == 0), drawing from the stream (seed, stream, 0): ok (0: the path ends here), t, weight, exited, the bounce
 *             count afterwards, and the stream's next number;
 *   tr        mediumTransmittance of the same ray with farT = max_t for (startOnSurface, endOnSurface) = (1,1), (1,0), (0,1), (0,0);
 *   phase     phaseEval(d, wo), then phaseSample(d) drawing from the stream (seed, stream, 1): w, pdf and the stream's next number.
 * Outputs behind a refused sampleDistance are unspecified.  TGHIP_E_INVALID (context left usable, nothing launched) for null pointers with n > 0, a
 * medium index outside TgHipSceneDesc::media, an index that names an operand entry of an `interpolated` medium (no medium of the scene: the entries
 * behind it do not exist for it to interpolate), a variant that is unknown or lacks the media code, a scene without media, or no scene; n == 0 succeeds
 * and launches nothing, as for the sibling entries. */
typedef struct TgHipMediumCase {
    int32_t  medium;          /* index in TgHipSceneDesc::media */
    uint32_t variant;         /* TGHIP_BSDF_VARIANT_* */
    uint32_t seed, stream;    /* the samplers: rngStart(seed, stream, 0) and (seed, stream, 1) */
    uint32_t state_bounce;    /* MediumState::bounce before the call */
    float    p[3], d[3];      /* the ray: origin, unit direction */
    float    max_t;           /* its far end; +inf allowed */
    float    wo[3];           /* a second unit direction, for phaseEval */
    uint32_t reserved;
} TgHipMediumCase;            /* 64 B */
typedef struct TgHipMediumResult {
    uint32_t ok;              /* mediumSampleDistance's return */
    float    t, weight[3];
    uint32_t exited;
    uint32_t bounce_after;
    float    tr[4][3];        /* [2*!startOnSurface + !endOnSurface][channel] */
    float    phase_f;
    float    w[3], phase_pdf;
    float    dist_next, phase_next;   /* the two streams' next numbers after the calls returned */
    uint32_t reserved[2];
} TgHipMediumResult;          /* 112 B */
int tghip_debug_medium(tghip_ctx *ctx, const TgHipMediumCase *cases, TgHipMediumResult *results, size_t n);
/* Which kernels a pass runs on a scene, as the context decides it once per upload, option and kind of pass (csrc/host/LaunchChoice.cpp; tungsten_host.h:
 * tgh_launch_choice answers the same without a device and documents the fields). */
#define TGHIP_KERNEL_NAME_LEN 80
typedef struct TgHipWalkLaunch {
    char name[TGHIP_KERNEL_NAME_LEN], sized_by[TGHIP_KERNEL_NAME_LEN];
    int32_t lds_formula, sized_lds_formula, max_threads, fixed_threads;
} TgHipWalkLaunch;
typedef struct TgHipShadeLaunch {
    char name[TGHIP_KERNEL_NAME_LEN];
    int32_t cls, variant;            /* the launch's class argument (4: the escaped paths, 5: class 0 and the escaped paths); TGHIP_BSDF_VARIANT_* of its family */
    uint32_t mask;                   /* the family's mask, with the Sobol' sampler's bit where the pass runs that twin */
    int32_t fuse, global_tables;     /* k_shade's FUSE bits and GLOBAL_TABLES */
    int32_t size, lane;              /* its workgroup size: shade_size[size] (0 simple, 1 complex, 2 all); "class_streams": 0 the part's stream, 1 / 2 beside it */
} TgHipShadeLaunch;
typedef struct TgHipShadeSize { char sized_by[TGHIP_KERNEL_NAME_LEN]; int32_t max_threads, fixed_threads; } TgHipShadeSize;
typedef struct TgHipLaunchChoice {
    int32_t flat, fused_flat, one_launch, paired, paired_inst, blocks_per_cu, parts;   /* parts: wanted, before the grid and the batch's items are asked */
    int32_t slot_cap, order_regs_cap, walk_arrays, fold_finish, nee_factors, camera_rays, tables_fit;
    TgHipWalkLaunch closest, shadow;                    /* empty names when fused_flat */
    int32_t num_shade, fused_pair, shade_launches;       /* entries of shade[]; the further class of k_shade_fused or 0; launches the counters book per iteration */
    TgHipShadeLaunch shade[6];
    TgHipShadeSize shade_size[3];
    int32_t tail_eligible, reserved;                     /* before the occupancy probe */
    char tail[TGHIP_KERNEL_NAME_LEN], tail_probe[TGHIP_KERNEL_NAME_LEN], camera_rays_name[TGHIP_KERNEL_NAME_LEN];
    int32_t ray_walk, reserved2;                         /* tghip_trace_rays / tghip_query_rays: 0 flat list, 1 BVH2, 2 instances, 3 wide BVH */
    char trace_rays[TGHIP_KERNEL_NAME_LEN];
} TgHipLaunchChoice;
/* What the context would launch for `pass` on the uploaded scene -- nothing is launched, no pool is allocated: the choice, the workgroup sizes the
 * occupancy of this device gives (threads_shade: simple / complex / all), the dynamic LDS bytes of the walk launches, the persistent grid, the parts the
 * loop runs as when the batch has items enough, and whether a workgroup of k_tail fits a CU.  TGHIP_E_INVALID for a pass tghip_render_pass refuses. */
typedef struct TgHipLaunchPlan {
    TgHipLaunchChoice choice;
    int32_t threads_closest, threads_shadow, threads_shade[3], threads_tail;
    uint32_t lds_closest, lds_shadow, lds_tail;
    uint32_t grid;
    int32_t parts, tail_fits;
} TgHipLaunchPlan;
int tghip_debug_launch_plan(tghip_ctx *ctx, const TgHipPassDesc *pass, TgHipLaunchPlan *out);
int tghip_set_option(tghip_ctx *ctx, const char *key, long long value);  /* "count_traversal", "max_slots", ...; "top_tree" = 0 before an upload:
                                                                             TgHipSceneDesc::top_nodes is ignored, flat lists are walked in record order.
                                                                             Instrumentation that never changes an image (tests hold that): "lds_tables" = 0
                                                                             shades as if the small tables did not fit the LDS copy, "env_lds" = 0 samples the
                                                                             environment map through its global tables, "hoist_quad" = 0 leaves a scene's one
                                                                             quad inside the walks, "tail_family" = 0 runs the all-types tail kernel.
                                                                             "shade_fused" (default 1): single-level scenes with class 0 and one further shading
                                                                             class shade an iteration in ONE launch (k_shade_fused); 0 = one launch per class, the
                                                                             same image bit for bit.  TgHipCounters::launches_shade counts every shading launch.
                                                                             Round 6, instanced scenes: "inst_wide" = 0 walks masters through their BVH2 (round 5's
                                                                             kernel; images differ only where two triangles of a master answer a ray one rounding
                                                                             apart), "inst_phase_min" / "inst_refill_at" the phase vote's threshold and the refill
                                                                             level of k_trace_closest_instw, "inst_shadow_fast" = 0 shadow rays on
                                                                             k_trace_shadow_wide<., ., INST> */
int tghip_get_counters(tghip_ctx *ctx, TgHipCounters *out);
int tghip_reset_counters(tghip_ctx *ctx);
/* Instrumentation (no reference analogue; bench.py roofline.valu.walk, profiles/r6_lane_util.json): the tallies the counting variants of the
 * two wide walks keep ("count_traversal" = 1), summed over every wave launch since the last tghip_reset_counters.  walk 0 = closest hit, 1 = shadow.
 * out[0..n): [0..3] wave time in 10-ns ticks (queue expansion, loop with queue, loop after the queue ran dry, wait + write-back), [4] wave launches,
 * [5] / [6] loop turns before / after dry, [7] / [8] busy lanes summed over those turns, [9] / [10] walks suspended / resumed, [11] longest loop,
 * [12] / [13] turns that ran the record test / lanes with a record in them, [14] / [15] the same for the node visit, [16] / [17] refill blocks run /
 * lanes refilled, [18] / [19] publish (NEE-term) blocks run / lanes in them, [20] record tests accepted, [21] rays walked.  Instanced scenes (walk 0):
 * [22] wave launches of k_trace_closest_instw (0: k_trace_closest_inst ran), [23] wide nodes visited inside masters, [24 + 2 k] / [25 + 2 k] runs / lanes
 * of section k of the turn (pt_wavefront.h lists the twelve sections of either kernel; bench.py: walk_summary names them).  Returns the number of
 * values written (<= n), or a negative error. */
int tghip_get_walk_stats(tghip_ctx *ctx, int walk, uint64_t *out, int n);

#ifdef __cplusplus
}
#endif
#endif /* TUNGSTEN_HIP_H_ */
