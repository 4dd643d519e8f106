// What tghip_query_radiance decides about a call before anything touches the device: the refusals of a malformed description, of missing or
// misaligned arrays and of a batch past what a pass holds; the virtual image whose pixels are the rays; the pass that renders it.  Plain host
// arithmetic over TgHipRadianceQueryDesc and the pointers' values -- nothing is read through them --: no device, no context
// (include/tungsten_host.h: tgh_query_radiance_check runs the check on its own, tools/radiance_query_check.cpp all of it under the sanitizers).
#ifndef TGAMD_RADIANCEQUERY_HPP_
#define TGAMD_RADIANCEQUERY_HPP_

#include "PassPlan.hpp"

#include <cstddef>
#include <string>

// TGHIP_OK; TGHIP_E_INVALID or -- a batch of 2^32 samples or more -- TGHIP_E_UNSUPPORTED with the refusal in `error`
int checkRadianceQuery(const TgHipRadianceQueryDesc *desc, const void *rays, const void *rgbSum, const void *count, size_t n, bool sceneHasSobol,
                       std::string &error);

// The virtual image of a batch of n >= 1 rays: width x height pixels, width*height >= n, the row-major pixel index IS the ray index, and the
// pixels past the last ray (the padding, fewer than one row) are the end of the last row.
#define RADIANCE_QUERY_WIDTH 16u           /* one tile column: a 16 x 16 tile is 256 consecutive rays */
struct RadianceQueryImage { uint32_t width, height; };
RadianceQueryImage radianceQueryImage(size_t n);

// The pass over that image a checked call stands for: the sample range, the seed and TGHIP_PASS_SOBOL from the description, one shard, no
// records.  tile_seeds stays NULL: every tile of the virtual image has the seed desc.sobol_seed, which the caller of planPass puts on the device.
TgHipPassDesc radianceQueryPass(const TgHipRadianceQueryDesc &desc);
// planPass (PassPlan.cpp) of that pass for that image: TGHIP_OK and the plan, or planPass's refusal
int planRadianceQuery(const TgHipRadianceQueryDesc &desc, size_t n, const PassPlanOptions &opt, PassPlan &out, std::string &error);

#endif
