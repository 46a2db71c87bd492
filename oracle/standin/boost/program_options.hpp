/*
 * Stand-in for the option map the reference consults through g_parameters:
 * every option is absent.  TEST INFRASTRUCTURE ONLY; written for
 * oracle/Makefile's `ref` rule, holds no behaviour beyond "not set".
 */
#ifndef KGX_STANDIN_BOOST_PROGRAM_OPTIONS_HPP
#define KGX_STANDIN_BOOST_PROGRAM_OPTIONS_HPP

#include <cstddef>
#include <string>

namespace boost { namespace program_options {

class variable_value {
public:
    template <class T> T as() const { return T(); }
};

class variables_map {
public:
    std::size_t count(const std::string &) const { return 0; }
    variable_value operator[](const std::string &) const { return variable_value(); }
};

} }

#endif
