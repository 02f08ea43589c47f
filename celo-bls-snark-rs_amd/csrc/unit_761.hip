#include "msm_unit.h"
template struct celo::MsmApi<celo::G_761>;
