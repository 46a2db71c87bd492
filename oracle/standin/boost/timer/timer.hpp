/*
 * Stand-in for the one name the reference's global.h takes from the timer
 * library: a type for its g_timer global.  TEST INFRASTRUCTURE ONLY; written
 * for oracle/Makefile's `ref` rule, holds no behaviour.
 */
#ifndef KGX_STANDIN_BOOST_TIMER_HPP
#define KGX_STANDIN_BOOST_TIMER_HPP

namespace boost { namespace timer {
class cpu_timer {};
} }

#endif
