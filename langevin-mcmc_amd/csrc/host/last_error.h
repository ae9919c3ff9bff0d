// The message behind lmc_last_error() (thread-local, host/context.cpp), for the host units beside context.cpp that implement ABI calls.
#pragma once
#include <string>

void LmcSetLastError(const std::string &what);
