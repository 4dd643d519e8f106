// What tghip_query_transmittance decides about a call before anything touches the device: the refusals of a malformed description, of missing or
// misaligned arrays, of a batch past 2^31 - 1 rays and of a start medium or an end cap the uploaded scene does not have.  Plain host arithmetic over
// TgHipTransmittanceQueryDesc, the pointers' values -- nothing is read through them -- and two small tables of the scene: no device, no context
// (include/tungsten_host.h: tgh_query_transmittance_check runs it on its own).
#ifndef TGAMD_TRANSMITTANCEQUERY_HPP_
#define TGAMD_TRANSMITTANCEQUERY_HPP_

#include "../../../include/tungsten_host.h"

#include <cstddef>
#include <string>

// TGHIP_OK, or TGHIP_E_INVALID with the refusal in `error`.  scene: see TgHostTransmittanceScene; nullptr = no media, no objects.
int checkTransmittanceQuery(const TgHipTransmittanceQueryDesc *desc, const void *rays, const void *media, const void *out, size_t n,
                            const TgHostTransmittanceScene *scene, std::string &error);

#endif
