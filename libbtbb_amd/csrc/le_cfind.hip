// le_cfind.hip -- the promiscuous LE Coded connection discovery as a translation unit of its own (le_cfind.h says why)
#include "le_cfind.h"
