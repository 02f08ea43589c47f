#include "msm_unit.h"
template struct celo::MsmAuxApi<celo::G2_377>;
