// cluster_host.hpp — what every entry point that takes mtd_cluster_params refuses before a device is touched (host only; cluster.hip and
// the units that run the cluster pass between their own launches: steinhardt_local.hip, coordination.hip, tetrahedral.hip)
#pragma once

#include "mtd_abi.h"

#include <cmath>

namespace mtd
{
// the option is on at all: "off" is the business of the caller, mtd_cluster_largest itself refuses it
inline bool cluster_on(const mtd_cluster_params *p) { return p && p->on; }

// MTD_ERR_INVALID_ARGUMENT for p == NULL, on == 0, r_link <= 0 or not finite, v_min not finite
inline int cluster_refuse(const mtd_cluster_params *p)
    {
    if (!cluster_on(p)) return MTD_ERR_INVALID_ARGUMENT;
    if (!(p->r_link > 0.0) || !std::isfinite(p->r_link) || !std::isfinite(p->v_min)) return MTD_ERR_INVALID_ARGUMENT;
    return MTD_SUCCESS;
    }
}
