// le_coded.hip -- the LE Coded PHY scan and decoder as a translation unit of their own (le_coded.h says why)
#include "le_coded.h"
