// What tghip_query_direct decides about a call before anything touches the device: the refusals of a malformed description, of missing or misaligned
// arrays, of a batch past 2^31 - 1 rays or 2^32 - 1 (ray, sample) items and of a start medium or a light the uploaded scene does not have.  Plain host
// arithmetic over TgHipDirectQueryDesc, the pointers' values -- nothing is read through them -- and a few facts of the scene: no device, no context
// (include/tungsten_host.h: tgh_query_direct_check runs it on its own).
#ifndef TGAMD_DIRECTQUERY_HPP_
#define TGAMD_DIRECTQUERY_HPP_

#include "../../../include/tungsten_host.h"

#include <cstddef>
#include <string>

// TGHIP_OK, TGHIP_E_INVALID or TGHIP_E_UNSUPPORTED with the refusal in `error`.  scene: see TgHostDirectScene; nullptr = no media, no lights, the
// camera in no medium.
int checkDirectQuery(const TgHipDirectQueryDesc *desc, const void *rays, const void *media, const void *out, size_t n, const TgHostDirectScene *scene,
                     std::string &error);

#endif
