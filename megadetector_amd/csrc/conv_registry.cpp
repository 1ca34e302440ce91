// The conv kernel registry of one storage type: the families in id order (mdhip_internal.h: ConvFamilyId, ConvRegistry).
// Host code only.

#include "mdhip_internal.h"

namespace mdhip {
namespace MDHIP_ST {

#if !defined(__HIP_DEVICE_COMPILE__)   // a host object: the device code object gets no copy of it
extern const ConvRegistry conv_registry = {{&conv_igemm, &conv_v2, &conv_v5, &conv_v5s, &conv_v5c, &conv_v6, &conv_f8, &conv_v7}};
#endif

}  // namespace MDHIP_ST
}  // namespace mdhip
